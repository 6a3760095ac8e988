// fsk_processor_remap_api.hip -- C ABI of libfskhip.so (include/fskhip_next.h): fskhip_processor_remap, and processor snapshots
// (fskhip_processor_snapshot_bytes / _snapshot / _snapshot_info_get, fskhip_processor_restore).  They carry the FSKProcessor row
// -- RX rings, pending modulations, `completed` counts -- where fskhip_remap_streams and the stream snapshots carry the FSKCore
// below it.  The image's format is documented in the header; this file is its only reader and writer.  Kernels:
// fsk_processor_remap.hip; the frame of an image (checksum, open front and back, selection and room checks) and the slab
// pipelines: fsk_stage.h, shared with the stream snapshots.
#include <algorithm>
#include <vector>

#include "fsk_engine.h"
#include "fsk_launch.h"
#include "fsk_proc.h"
#include "fsk_stage.h"

using namespace fsk;

namespace {

constexpr uint32_t kProcMagic = 0x504B5346u;   // "FSKP"
constexpr uint32_t kProcFormat = 1;

struct ProcHeader {
  uint32_t magic, format;
  uint32_t header_bytes, record_bytes;
  uint32_t n_records;
  uint32_t rx_capacity, payload_capacity;   // a record: kProcRecFixed + payload_capacity + rx_capacity rounded up to 16
  uint32_t zero0;
  uint64_t checksum;                        // snap_sum over the header with this field 0, then the records
  uint64_t zero1;
};
static_assert(sizeof(ProcHeader) == 48 && sizeof(ProcHeader) % 16 == 0, "ProcHeader has padding");

uint32_t ring_pitch_of(uint32_t rx_capacity) { return (rx_capacity + 15u) & ~15u; }
uint32_t record_bytes_of(uint32_t rx_capacity, uint32_t pay_cap) { return kProcRecFixed + pay_cap + ring_pitch_of(rx_capacity); }

// a validated image: the header (copied: the caller's bytes need no alignment) and the records
struct ProcSnap {
  ProcHeader h;
  const unsigned char *rec;
};

int proc_open(const char *who, const void *buf, size_t size, ProcSnap *s) {
  ProcHeader &h = s->h;
  if (const int rc = image_open_front(who, "processor snapshot", buf, size, kProcMagic, kProcFormat, &h)) return rc;
  if (h.rx_capacity == 0 || h.rx_capacity > (1u << 30)) return fail(FSKHIP_E_INVALID, "%s: rx_capacity %u in the snapshot", who, h.rx_capacity);
  if ((h.payload_capacity & 15u) != 0u || h.payload_capacity > (1u << 30))
    return fail(FSKHIP_E_INVALID, "%s: payload_capacity %u in the snapshot (a multiple of 16)", who, h.payload_capacity);
  if (h.record_bytes != record_bytes_of(h.rx_capacity, h.payload_capacity))
    return fail(FSKHIP_E_INVALID, "%s: record_bytes %u, but rx_capacity %u and payload_capacity %u make records of %u bytes", who, h.record_bytes, h.rx_capacity,
                h.payload_capacity, record_bytes_of(h.rx_capacity, h.payload_capacity));
  if (const int rc = image_open_back(who, "n_records", buf, size, h, h.n_records, &s->rec)) return rc;
  // the words a kernel would index with: inside the ring, inside the record's payload
  for (uint32_t r = 0; r < h.n_records; r++) {
    uint32_t w[8];
    std::memcpy(w, s->rec + (size_t)r * h.record_bytes, sizeof(w));
    if (w[0] >= h.rx_capacity || w[1] >= h.rx_capacity || w[2] > h.rx_capacity)
      return fail(FSKHIP_E_INVALID, "%s: record %u: ring words (writeIndex %u, readIndex %u, _length %u) outside rx_capacity %u", who, r, w[0], w[1], w[2], h.rx_capacity);
    if (w[3] > 1u || w[7] > h.payload_capacity || (w[6] != 0u && w[5] >= w[6]))
      return fail(FSKHIP_E_INVALID, "%s: record %u: modulator words (pending %u, position %u of %u, payload %u bytes of %u) are inconsistent", who, r, w[3], w[5], w[6], w[7],
                  h.payload_capacity);
  }
  return FSKHIP_OK;
}

// the longest pending payload among streams idx[0 .. n) of p (idx null: all its streams; -1 entries skipped).  After the
// caller's device synchronisation; p is read only.
int max_pending_payload(const char *who, const fskhip_processor *p, const int64_t *idx, uint32_t n, uint32_t *out) {
  int64_t *d_idx = nullptr;
  uint32_t *d_out = nullptr;
  hipError_t err = hipMalloc((void **)&d_out, sizeof(uint32_t));
  if (err == hipSuccess && idx && n) err = hipMalloc((void **)&d_idx, sizeof(int64_t) * n);
  if (err == hipSuccess && d_idx) err = hipMemcpy(d_idx, idx, sizeof(int64_t) * n, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = launch_processor_max_payload(p->T, d_idx, idx ? n : p->S, d_out, nullptr);
  if (err == hipSuccess) err = hipMemcpy(out, d_out, sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (d_idx) (void)hipFree(d_idx);
  if (d_out) (void)hipFree(d_out);
  if (err != hipSuccess) return fail(FSKHIP_E_HIP, "%s: %s", who, hipGetErrorString(err));
  return FSKHIP_OK;
}

// what fskhip_processor_remap and fskhip_processor_restore ask of their destination and map
int check_dst(const char *who, const fskhip_processor *dst, const char *the, const char *unit, uint32_t n_src, uint32_t src_rx_capacity, const int64_t *map, uint32_t n_map) {
  if (n_map != dst->S) return fail(FSKHIP_E_INVALID, "%s: n_map %u != the destination's %u streams", who, n_map, dst->S);
  if (dst->T.rx_cap != src_rx_capacity) return fail(FSKHIP_E_INVALID, "%s: rx_capacity differs (the destination's %u, %s's %u)", who, dst->T.rx_cap, the, src_rx_capacity);
  if (dst->used) return fail(FSKHIP_E_INVALID, "%s: the destination has been used already (process, modulate, drain or reset: remap into a freshly created processor)", who);
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] >= (int64_t)n_src) return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld, %s has %u %s", who, i, (long long)map[i], the, n_src, unit);
  return FSKHIP_OK;
}

}  // namespace

extern "C" {

int fskhip_processor_remap(fskhip_processor *dst, const fskhip_processor *src, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_processor_remap";
  if (!dst || !src) return fail(FSKHIP_E_INVALID, "%s: null processor", who);
  if (dst == src) return fail(FSKHIP_E_INVALID, "%s: dst and src are the same processor", who);
  if (const int rc = remap_check_map(who, "a source stream", map, n_map)) return rc;
  if (dst->device != src->device) return fail(FSKHIP_E_INVALID, "%s: the processors are on different devices (%d, %d): use a snapshot", who, dst->device, src->device);
  if (const int rc = check_dst(who, dst, "the source", "streams", src->S, src->T.rx_cap, map, n_map)) return rc;
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] >= 0 && !config_all_fields_equal(engine_stream_config(dst->e, i), engine_stream_config(src->e, (size_t)map[i])))
      return fail(FSKHIP_E_INVALID, "%s: the config of stream %u differs from that of source stream %lld", who, i, (long long)map[i]);
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t max_pay = 0;
  if (const int rc = max_pending_payload(who, src, map, n_map, &max_pay)) return rc;
  if (const int rc = processor_grow_payload(dst, max_pay)) return rc;
  if (n_map == 0) return FSKHIP_OK;
  int64_t *d_map = nullptr;
  HIP_TRY_AS(hipMalloc((void **)&d_map, sizeof(int64_t) * n_map), "hipMalloc(map)", true, (void)0);
  HIP_TRY_AS(hipMemcpy(d_map, map, sizeof(int64_t) * n_map, hipMemcpyHostToDevice), "hipMemcpy(map)", false, (void)hipFree(d_map));
  HIP_TRY_AS(launch_processor_gather(dst->T, dst->S, d_map, src->T, nullptr), "proc_gather_kernel", false, (void)hipFree(d_map));
  HIP_TRY_AS(hipDeviceSynchronize(), "hipDeviceSynchronize", false, (void)hipFree(d_map));
  (void)hipFree(d_map);
  return FSKHIP_OK;
}

size_t fskhip_processor_snapshot_bytes(const fskhip_processor *p, const int64_t *sel, uint32_t n_sel) {
  static const char who[] = "fskhip_processor_snapshot_bytes";
  if (!p) return 0;
  if (!sel) n_sel = p->S;
  if (check_sel(who, "processor", sel, n_sel, p->S)) return 0;
  if (hipSetDevice(p->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 0;
  uint32_t max_pay = 0;
  if (max_pending_payload(who, p, sel, n_sel, &max_pay)) return 0;
  return sizeof(ProcHeader) + (size_t)n_sel * record_bytes_of(p->T.rx_cap, (max_pay + 15u) & ~15u);
}

int fskhip_processor_snapshot(fskhip_processor *p, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written) {
  static const char who[] = "fskhip_processor_snapshot";
  if (!p) return fail(FSKHIP_E_INVALID, "%s: null processor", who);
  if (!sel) n_sel = p->S;
  if (const int rc = check_sel(who, "processor", sel, n_sel, p->S)) return rc;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t max_pay = 0;
  if (const int rc = max_pending_payload(who, p, sel, n_sel, &max_pay)) return rc;
  const uint32_t pay_cap = (max_pay + 15u) & ~15u;
  const size_t rec_bytes = record_bytes_of(p->T.rx_cap, pay_cap), need = sizeof(ProcHeader) + (size_t)n_sel * rec_bytes;
  if (const int rc = check_room(who, n_sel, need, buf, cap, written)) return rc;

  ProcHeader h = image_header<ProcHeader>(kProcMagic, kProcFormat, rec_bytes);
  h.n_records = n_sel; h.rx_capacity = p->T.rx_cap; h.payload_capacity = pay_cap;
  unsigned char *rec = (unsigned char *)buf + sizeof(ProcHeader);
  SnapSum sum;
  snap_sum(sum, &h, sizeof(h));   // (checksum field still 0)

  const auto pack = [&](const int64_t *d_sel, uint32_t first, uint32_t count, void *d_buf, hipStream_t stream) {
    const ProcImage I{nullptr, (uint32_t)rec_bytes, pay_cap, ring_pitch_of(p->T.rx_cap), first, count};
    return launch_processor_pack(p->T, d_sel, I, d_buf, stream);
  };
  // the host's part of a slab that has arrived: the checksum
  const auto finish = [&](uint32_t a, uint32_t b) { snap_sum(sum, rec + (size_t)a * rec_bytes, (size_t)(b - a) * rec_bytes); };
  if (const int rc = stage_records_out(who, p->stream, sel, n_sel, rec_bytes, rec, pack, finish)) return rc;
  h.checksum = snap_sum_value(sum);
  std::memcpy(buf, &h, sizeof(h));
  return FSKHIP_OK;
}

int fskhip_processor_snapshot_info_get(const void *buf, size_t size, fskhip_processor_snapshot_info *info) {
  static const char who[] = "fskhip_processor_snapshot_info_get";
  ProcSnap s;
  if (const int rc = proc_open(who, buf, size, &s)) return rc;
  if (!info) return fail(FSKHIP_E_INVALID, "%s: null info", who);
  std::memset(info, 0, sizeof(*info));
  info->n_streams = s.h.n_records; info->rx_capacity = s.h.rx_capacity; info->payload_capacity = s.h.payload_capacity;
  info->record_bytes = s.h.record_bytes;
  return FSKHIP_OK;
}

int fskhip_processor_restore(fskhip_processor *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_processor_restore";
  if (const int rc = remap_check_map(who, "a record of the snapshot", map, n_map)) return rc;
  ProcSnap s;
  if (const int rc = proc_open(who, buf, size, &s)) return rc;
  if (!dst) return fail(FSKHIP_E_INVALID, "%s: null processor", who);
  const ProcHeader &h = s.h;
  if (const int rc = check_dst(who, dst, "the snapshot", "records", h.n_records, h.rx_capacity, map, n_map)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = processor_grow_payload(dst, h.payload_capacity)) return rc;
  if (n_map == 0) return FSKHIP_OK;

  const auto unpack = [&](const int64_t *d_map, uint32_t first, uint32_t count, bool fresh_too, void *d_buf, hipStream_t stream) {
    const ProcImage I{(const uint8_t *)d_buf, h.record_bytes, h.payload_capacity, ring_pitch_of(h.rx_capacity), first, count};
    return launch_processor_unpack(dst->T, dst->S, d_map, I, fresh_too, stream);
  };
  return stage_records_in(who, dst->stream, map, n_map, s.rec, h.n_records, h.record_bytes, unpack);
}

}  // extern "C"
