// fsk_snapshot_api.hip -- C ABI of libfskhip.so (include/fskhip.h): stream snapshots.  A snapshot is a host-side image of a set
// of streams -- one SnapHeader, then fixed-size stream-major records -- that fskhip_restore_streams continues from under
// fskhip_remap_streams' contract, on any device and in any process running this build.  The format is documented in the
// header; this file is its only reader and writer.  The pack / unpack kernels are fsk_snapshot.hip's; the checks, the
// lock-step decision and the host-side counters are the remap's own (fsk_create.hip, fsk_engine.h); the frame of an image
// (checksum, open front and back, selection and room checks) and the slab pipelines are fsk_stage.h's, shared with the
// processor snapshots.
#include <algorithm>

#include "fsk_engine.h"
#include "fsk_launch.h"
#include "fsk_stage.h"

using namespace fsk;

namespace {

constexpr uint32_t kSnapMagic = 0x534B5346u;   // "FSKS"
constexpr uint32_t kSnapFormat = 1;

// fskhip_config without the padding its int32 / double mix leaves: every byte of a snapshot is defined
struct SnapConfig {
  double sampleRate, baudRate, markFrequency, spaceFrequency, syncThreshold, preFilterBandwidth;
  int32_t preamblePattern[FSKHIP_MAX_PATTERN_BYTES], sfdPattern[FSKHIP_MAX_PATTERN_BYTES];
  int32_t preambleLen, sfdLen, startBits, stopBits, parity, agcEnabled, adaptiveThreshold, zero;
};
static_assert(sizeof(SnapConfig) == 6 * 8 + (2 * FSKHIP_MAX_PATTERN_BYTES + 8) * 4, "SnapConfig has padding");

struct SnapHeader {
  uint32_t magic, format;
  uint32_t rf_count, if_count;    // the state-layout stamp: the field counts and ...
  uint64_t fields_hash;           // ... FNV-1a of the field names in fsk_params.h order (and the spans the fp32 reset words count in)
  uint64_t checksum;              // snap_sum over the header with this field 0, then the records
  uint32_t header_bytes, record_bytes;
  uint32_t n_streams;
  int32_t precision;
  uint32_t per_stream_configs;    // 0: every record runs under cfg0
  uint32_t d, amp_cap, wide, frac, n_bits, ring_cap;    // the geometry fskhip_remap_streams compares
  uint32_t ds_parity, ds_uniform, gen_odd, quality;     // engine-level values a destination takes over
  uint32_t grid_poly_phase, grid_amp_pos;               // the ring grid: source row 0's positions (every row's, in lock step)
  uint32_t frame_valid;           // fp32, one shared configuration, at least one stream: frame_phase is the engine's
  uint32_t zero[2];
  uint64_t frame_phase;           // the free-running I/Q frame: NCO phase minus frame offset of source row 0 (64-bit turns)
  uint64_t calls, total_samples, pushes;
  SnapConfig cfg0;
};
static_assert(sizeof(SnapHeader) == 352 && sizeof(SnapHeader) % 16 == 0, "SnapHeader has padding");

// the host part of a record (kSnapHostWords words): what of a stream lives on the host
struct SnapRecordHost {
  double markFrequency, spaceFrequency, preFilterBandwidth;
  uint32_t adaptiveThreshold, zero;
  uint64_t base_calls, base_samples;
};
static_assert(sizeof(SnapRecordHost) == kSnapHostWords * 4, "SnapRecordHost has padding");

uint64_t fields_hash() {
  static const char names[] =
#define X(n) #n ","
      FSK_REAL_FIELDS(X) FSK_REAL_FIELDS_PIPE(X) FSK_REAL_FIELDS_QUALITY(X) "|" FSK_INT_FIELDS(X) FSK_INT_FIELDS_PIPE(X) FSK_INT_FIELDS_QUALITY(X)
#undef X
      ;
  uint64_t h = 0xcbf29ce484222325ull;
  for (const char *p = names; *p; p++) h = (h ^ (uint8_t)*p) * 0x100000001b3ull;
  h = (h ^ kZeroLagPairs) * 0x100000001b3ull;
  h = (h ^ kHandLag) * 0x100000001b3ull;
  return h;
}

SnapConfig pack_config(const fskhip_config &c) {
  SnapConfig o;
  std::memset(&o, 0, sizeof(o));
  o.sampleRate = c.sampleRate; o.baudRate = c.baudRate; o.markFrequency = c.markFrequency; o.spaceFrequency = c.spaceFrequency;
  o.syncThreshold = c.syncThreshold; o.preFilterBandwidth = c.preFilterBandwidth;
  // (only the bytes in use: what lies behind preambleLen / sfdLen in the caller's struct is not state)
  for (int i = 0; i < FSKHIP_MAX_PATTERN_BYTES; i++) {
    o.preamblePattern[i] = i < c.preambleLen ? c.preamblePattern[i] : 0;
    o.sfdPattern[i] = i < c.sfdLen ? c.sfdPattern[i] : 0;
  }
  o.preambleLen = c.preambleLen; o.sfdLen = c.sfdLen; o.startBits = c.startBits; o.stopBits = c.stopBits; o.parity = c.parity;
  o.agcEnabled = c.agcEnabled != 0; o.adaptiveThreshold = c.adaptiveThreshold != 0;
  return o;
}
fskhip_config unpack_config(const SnapConfig &c) {
  fskhip_config o;
  std::memset(&o, 0, sizeof(o));
  o.sampleRate = c.sampleRate; o.baudRate = c.baudRate; o.markFrequency = c.markFrequency; o.spaceFrequency = c.spaceFrequency;
  o.syncThreshold = c.syncThreshold; o.preFilterBandwidth = c.preFilterBandwidth;
  std::memcpy(o.preamblePattern, c.preamblePattern, sizeof(o.preamblePattern));
  std::memcpy(o.sfdPattern, c.sfdPattern, sizeof(o.sfdPattern));
  o.preambleLen = c.preambleLen; o.sfdLen = c.sfdLen; o.startBits = c.startBits; o.stopBits = c.stopBits; o.parity = c.parity;
  o.agcEnabled = c.agcEnabled; o.adaptiveThreshold = c.adaptiveThreshold;
  return o;
}

// A validated snapshot: the header (copied: the caller's bytes need no alignment), its record layout and the records.
struct Snap {
  SnapHeader h;
  SnapLayout L;
  const unsigned char *rec;
  SnapRecordHost host_part(size_t i) const {
    SnapRecordHost r;
    std::memcpy(&r, rec + i * h.record_bytes, sizeof(r));
    return r;
  }
  fskhip_config config(size_t i) const {
    fskhip_config c = unpack_config(h.cfg0);
    const SnapRecordHost r = host_part(i);
    c.markFrequency = r.markFrequency; c.spaceFrequency = r.spaceFrequency; c.preFilterBandwidth = r.preFilterBandwidth;
    c.adaptiveThreshold = (int32_t)r.adaptiveThreshold;
    return c;
  }
  uint32_t int_word(size_t i, int f) const {   // IF_* word f of record i
    uint32_t w0 = 0, v;
    for (uint32_t k = 0; k < L.n_sec; k++)
      if (L.sec[k].kind == SNAP_IF) w0 = L.sec[k].w0;
    std::memcpy(&v, rec + i * h.record_bytes + 4u * (w0 + (uint32_t)f), 4);
    return v;
  }
};

int snap_open(const char *who, const void *buf, size_t size, Snap *s) {
  SnapHeader &h = s->h;
  const auto stamp = [&] {
    if (h.rf_count != RF_COUNT || h.if_count != IF_COUNT || h.fields_hash != fields_hash())
      return fail(FSKHIP_E_INVALID, "%s: the snapshot's state layout (%u + %u words, stamp %016llx) is another build's (%d + %d words, stamp %016llx)", who, h.rf_count,
                  h.if_count, (unsigned long long)h.fields_hash, (int)RF_COUNT, (int)IF_COUNT, (unsigned long long)fields_hash());
    return (int)FSKHIP_OK;
  };
  if (const int rc = image_open_front(who, "snapshot", buf, size, kSnapMagic, kSnapFormat, &h, stamp)) return rc;
  if (h.precision != FSKHIP_PRECISION_F32 && h.precision != FSKHIP_PRECISION_F64) return fail(FSKHIP_E_INVALID, "%s: unknown precision %d in the snapshot", who, h.precision);
  if (h.amp_cap != 8u * h.d || h.d == 0 || h.d > (1u << 20) || h.wide > 1 || h.frac > 1 || (h.frac && !h.wide))
    return fail(FSKHIP_E_INVALID, "%s: inconsistent geometry in the snapshot (d %u, amp_cap %u, wide %u, frac %u)", who, h.d, h.amp_cap, h.wide, h.frac);
  s->L = snap_layout(h.precision, h.d, h.amp_cap, h.wide, h.frac);
  if (h.record_bytes != 4u * s->L.rec_words)
    return fail(FSKHIP_E_INVALID, "%s: record_bytes %u, but this geometry and precision make records of %u bytes", who, h.record_bytes, 4u * s->L.rec_words);
  return image_open_back(who, "n_streams", buf, size, h, h.n_streams, &s->rec);
}

}  // namespace

extern "C" {

size_t fskhip_snapshot_bytes(const fskhip_engine *e, uint32_t n_sel) {
  if (!e) return 0;
  const SnapLayout L = snap_layout(e->precision, e->P.d, e->P.amp_cap, e->P.wide, e->P.frac);
  return sizeof(SnapHeader) + (size_t)n_sel * 4u * L.rec_words;
}

int fskhip_snapshot_streams(fskhip_engine *e, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written) {
  static const char who[] = "fskhip_snapshot_streams";
  if (!e) return fail(FSKHIP_E_INVALID, "%s: null engine", who);
  if (!sel) n_sel = e->n_streams;
  if (const int rc = check_sel(who, "engine", sel, n_sel, e->n_streams)) return rc;
  const SnapLayout L = snap_layout(e->precision, e->P.d, e->P.amp_cap, e->P.wide, e->P.frac);
  const size_t rec_bytes = 4u * (size_t)L.rec_words, need = sizeof(SnapHeader) + (size_t)n_sel * rec_bytes;
  if (const int rc = check_room(who, n_sel, need, buf, cap, written)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = engine_refuse_handoff(who, "the engine", e)) return rc;

  SnapHeader h = image_header<SnapHeader>(kSnapMagic, kSnapFormat, rec_bytes);
  h.rf_count = RF_COUNT; h.if_count = IF_COUNT; h.fields_hash = fields_hash();
  h.n_streams = n_sel; h.precision = e->precision;
  h.per_stream_configs = e->cfgs.size() == 1 ? 0u : 1u;
  h.d = e->P.d; h.amp_cap = e->P.amp_cap; h.wide = e->P.wide; h.frac = e->P.frac; h.n_bits = e->P.n_bits; h.ring_cap = e->P.ring_cap;
  h.ds_parity = e->ds_parity; h.ds_uniform = e->ds_uniform ? 1u : 0u; h.gen_odd = e->gen_odd ? 1u : 0u; h.quality = e->P.quality;
  h.calls = e->calls; h.total_samples = e->total_samples; h.pushes = e->pushes;
  h.cfg0 = pack_config(e->cfg0);
  {   // row 0's ring positions and frame words: what new streams of a restore take from "the source", whichever streams are selected
    const int rows[6] = {IF_poly_phase, IF_amp_pos, IF_nco_lo, IF_nco_hi, IF_fr_lo, IF_fr_hi};
    uint32_t w[6];
    for (int k = 0; k < 6; k++) HIP_TRY(hipMemcpy(&w[k], e->S.is + (size_t)rows[k] * e->n_streams, sizeof(uint32_t), hipMemcpyDeviceToHost));
    h.grid_poly_phase = w[0]; h.grid_amp_pos = w[1];
    h.frame_valid = (e->precision == FSKHIP_PRECISION_F32 && e->P.uni_cfg) ? 1u : 0u;
    h.frame_phase = h.frame_valid ? frame_phase(w[2], w[3], w[4], w[5]) : 0ull;
  }
  unsigned char *rec = (unsigned char *)buf + sizeof(SnapHeader);
  SnapSum sum;
  snap_sum(sum, &h, sizeof(h));   // (checksum field still 0)

  const auto pack = [&](const int64_t *d_sel, uint32_t first, uint32_t count, void *d_buf, hipStream_t stream) {
    return launch_snap_pack(L, e->S, e->n_streams, d_sel, first, count, d_buf, stream);
  };
  // the host's part of a slab that has arrived: the records' host parts, the checksum
  const auto finish = [&](uint32_t a, uint32_t b) {
    for (uint32_t r = a; r < b; r++) {
      const size_t s = sel ? (size_t)sel[r] : r;
      const fskhip_config &c = engine_stream_config(e, s);
      SnapRecordHost hp;
      std::memset(&hp, 0, sizeof(hp));
      hp.markFrequency = c.markFrequency; hp.spaceFrequency = c.spaceFrequency; hp.preFilterBandwidth = c.preFilterBandwidth;
      hp.adaptiveThreshold = c.adaptiveThreshold != 0;
      hp.base_calls = e->base_calls[s]; hp.base_samples = e->base_samples[s];
      std::memcpy(rec + (size_t)r * rec_bytes, &hp, sizeof(hp));
    }
    snap_sum(sum, rec + (size_t)a * rec_bytes, (size_t)(b - a) * rec_bytes);
  };
  if (const int rc = stage_records_out(who, e->host.stream, sel, n_sel, rec_bytes, rec, pack, finish)) return rc;
  h.checksum = snap_sum_value(sum);
  std::memcpy(buf, &h, sizeof(h));
  return FSKHIP_OK;
}

int fskhip_snapshot_info_get(const void *buf, size_t size, fskhip_snapshot_info *info) {
  static const char who[] = "fskhip_snapshot_info_get";
  Snap s;
  if (const int rc = snap_open(who, buf, size, &s)) return rc;
  if (!info) return fail(FSKHIP_E_INVALID, "%s: null info", who);
  std::memset(info, 0, sizeof(*info));
  info->n_streams = s.h.n_streams; info->precision = s.h.precision; info->per_stream_configs = s.h.per_stream_configs;
  info->record_bytes = s.h.record_bytes;
  info->demodulationCalls = (double)s.h.calls; info->totalSamplesProcessed = (double)s.h.total_samples;
  return FSKHIP_OK;
}

int fskhip_snapshot_stream_config(const void *buf, size_t size, uint32_t i, fskhip_config *cfg) {
  static const char who[] = "fskhip_snapshot_stream_config";
  Snap s;
  if (const int rc = snap_open(who, buf, size, &s)) return rc;
  if (!cfg) return fail(FSKHIP_E_INVALID, "%s: null cfg", who);
  // (record 0 of an empty snapshot: the shared configuration, so that a host can still build the destination from the file)
  if (i >= s.h.n_streams && !(i == 0 && s.h.n_streams == 0)) return fail(FSKHIP_E_INVALID, "%s: record %u, the snapshot has %u", who, i, s.h.n_streams);
  *cfg = s.h.n_streams ? s.config(i) : unpack_config(s.h.cfg0);
  return FSKHIP_OK;
}

int fskhip_snapshot_concat(const void *const *bufs, const size_t *sizes, uint32_t n, void *out, size_t cap, size_t *written) {
  static const char who[] = "fskhip_snapshot_concat";
  if (!bufs || !sizes || n == 0) return fail(FSKHIP_E_INVALID, "%s: null / no snapshots", who);
  std::vector<Snap> ss(n);
  for (uint32_t k = 0; k < n; k++)
    if (const int rc = snap_open(who, bufs[k], sizes[k], &ss[k])) {
      const std::string msg = fskhip_last_error();
      return fail(rc, "%s (snapshot %u)", msg.c_str(), k);
    }
  SnapHeader h = ss[0].h;
  size_t total = 0;
  for (uint32_t k = 0; k < n; k++) {
    const SnapHeader &g = ss[k].h;
    total += g.n_streams;
#define SAME(field, fmt, cast)                                                                                                                        \
  if (g.field != h.field)                                                                                                                             \
    return fail(FSKHIP_E_INVALID, "%s: snapshots 0 and %u differ in %s (" fmt ", " fmt "): not images of what could have been one engine", who, k, #field, \
                (cast)h.field, (cast)g.field)
    SAME(precision, "%d", int);
    if (!config_shared_fields_equal(unpack_config(h.cfg0), unpack_config(g.cfg0)))
      return fail(FSKHIP_E_INVALID, "%s: snapshots 0 and %u differ in the shared configuration (sampleRate, baudRate, framing, patterns, syncThreshold, agcEnabled)", who, k);
    SAME(d, "%u", unsigned); SAME(amp_cap, "%u", unsigned); SAME(wide, "%u", unsigned); SAME(frac, "%u", unsigned); SAME(n_bits, "%u", unsigned);
    SAME(ring_cap, "%u", unsigned);
    SAME(calls, "%llu", unsigned long long); SAME(total_samples, "%llu", unsigned long long); SAME(pushes, "%llu", unsigned long long);
    SAME(ds_parity, "%u", unsigned); SAME(ds_uniform, "%u", unsigned); SAME(gen_odd, "%u", unsigned); SAME(quality, "%u", unsigned);
    if (h.ds_uniform && !h.frac) { SAME(grid_poly_phase, "%u", unsigned); SAME(grid_amp_pos, "%u", unsigned); }
    if (h.frame_valid && g.frame_valid) SAME(frame_phase, "%llu", unsigned long long);
#undef SAME
    // one shared configuration only if every part had it, and the same one
    const fskhip_config a = unpack_config(h.cfg0), b = unpack_config(g.cfg0);
    if (g.per_stream_configs || a.markFrequency != b.markFrequency || a.spaceFrequency != b.spaceFrequency || a.preFilterBandwidth != b.preFilterBandwidth ||
        a.adaptiveThreshold != b.adaptiveThreshold)
      h.per_stream_configs = 1;
    if (!g.frame_valid) h.frame_valid = 0;
  }
  if (h.per_stream_configs) h.frame_valid = 0;
  if (!h.frame_valid) h.frame_phase = 0;
  if (total > 0xFFFFFFFFull) return fail(FSKHIP_E_INVALID, "%s: %zu streams in all", who, total);
  const size_t need = sizeof(SnapHeader) + total * h.record_bytes;
  if (written) *written = need;
  if (!out || cap < need) return fail(FSKHIP_E_OVERFLOW, "%s: the snapshots take %zu bytes together, the buffer has %zu", who, need, out ? cap : (size_t)0);
  h.n_streams = (uint32_t)total;
  unsigned char *rec = (unsigned char *)out + sizeof(SnapHeader);
  size_t at = 0;
  for (uint32_t k = 0; k < n; k++) {
    const size_t bytes = (size_t)ss[k].h.n_streams * h.record_bytes;
    if (bytes) std::memmove(rec + at, ss[k].rec, bytes);
    at += bytes;
  }
  h.checksum = image_checksum(h, rec, at);
  std::memcpy(out, &h, sizeof(h));
  return FSKHIP_OK;
}

int fskhip_restore_streams(fskhip_engine *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_restore_streams";
  if (const int rc = remap_check_map(who, "a record of the snapshot", map, n_map)) return rc;
  Snap s;
  if (const int rc = snap_open(who, buf, size, &s)) return rc;
  if (!dst) return fail(FSKHIP_E_INVALID, "%s: null engine", who);
  const SnapHeader &h = s.h;
  StreamSource V{};
  V.who = who; V.the = "the snapshot"; V.unit = "records"; V.item = "snapshot record";
  V.precision = h.precision; V.n_streams = h.n_streams; V.cfg0 = unpack_config(h.cfg0);
  V.d = h.d; V.amp_cap = h.amp_cap; V.wide = h.wide; V.frac = h.frac; V.n_bits = h.n_bits; V.ring_cap = h.ring_cap;
  V.calls = h.calls; V.total_samples = h.total_samples; V.pushes = h.pushes;
  V.ds_parity = h.ds_parity; V.ds_uniform = h.ds_uniform != 0; V.gen_odd = h.gen_odd != 0; V.quality = h.quality;
  V.ctx = &s;
  V.config = [](const void *ctx, size_t i) { return ((const Snap *)ctx)->config(i); };
  V.baselines = [](const void *ctx, size_t i, uint64_t *calls, uint64_t *samples) {
    const SnapRecordHost r = ((const Snap *)ctx)->host_part(i);
    *calls = r.base_calls; *samples = r.base_samples;
  };
  RemapPlan plan{};
  if (const int rc = remap_check(dst, V, map, n_map, &plan)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());

  NewStream N{};
  N.matched_zero = dst->matched_zero;
  N.grid = plan.grid ? 1u : 0u; N.poly_phase = h.grid_poly_phase; N.amp_pos = h.grid_amp_pos;
  N.frame = plan.frame ? 1u : 0u;
  if (plan.frame) {
    const size_t r = (size_t)plan.frame_row;
    N.fr0 = frame_phase(s.int_word(r, IF_nco_lo), s.int_word(r, IF_nco_hi), s.int_word(r, IF_fr_lo), s.int_word(r, IF_fr_hi));
  }
  const auto unpack = [&](const int64_t *d_map, uint32_t first, uint32_t count, bool fresh_too, void *d_buf, hipStream_t stream) {
    return launch_snap_unpack(dst->precision, s.L, dst->S, dst->n_streams, d_map, first, count, fresh_too, N, d_buf, stream);
  };
  if (const int rc = stage_records_in(who, dst->host.stream, map, n_map, s.rec, h.n_streams, h.record_bytes, unpack)) return rc;
  remap_finish(dst, V, map, n_map, plan);
  return FSKHIP_OK;
}

}  // extern "C"
