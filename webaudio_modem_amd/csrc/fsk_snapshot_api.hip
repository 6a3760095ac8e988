// fsk_snapshot_api.hip -- C ABI of libfskhip.so (include/fskhip.h): stream snapshots.  A snapshot is a host-side image of a set
// of streams -- one SnapHeader, then fixed-size stream-major records -- that fskhip_restore_streams continues from under
// fskhip_remap_streams' contract, on any device and in any process running this build.  The format is documented in the
// header; its layout and the one definition of a valid image are fsk_snapshot_image.h's (host-only, on fsk_image.h's frame), and
// this file is the format's only writer.  The pack / unpack kernels are fsk_snapshot.hip's; the checks, the lock-step decision
// and the host-side counters are the remap's own (fsk_create.hip, fsk_engine.h); the selection and room checks and the slab
// pipelines are fsk_stage.h's, shared with the other three snapshot units.
#include <algorithm>

#include "fsk_engine.h"
#include "fsk_launch.h"
#include "fsk_snapshot_image.h"
#include "fsk_stage.h"

using namespace fsk;

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

  SnapHeader h = image_header<SnapHeader>(kSnapMagic, kSnapFormat);
  h.rf_count = RF_COUNT; h.if_count = IF_COUNT; h.fields_hash = fields_hash();
  h.record_bytes = (uint32_t)rec_bytes; h.n_streams = n_sel; h.precision = e->precision;
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
  if (const int rc = open_image(who, snap_image_open, buf, size, &s)) return rc;
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
  if (const int rc = open_image(who, snap_image_open, buf, size, &s)) return rc;
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
    if (const int rc = open_image(who, snap_image_open, bufs[k], sizes[k], &ss[k])) {
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
  image_seal(h, out, need);
  return FSKHIP_OK;
}

int fskhip_restore_streams(fskhip_engine *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_restore_streams";
  if (const int rc = remap_check_map(who, "a record of the snapshot", map, n_map)) return rc;
  Snap s;
  if (const int rc = open_image(who, snap_image_open, buf, size, &s)) return rc;
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
