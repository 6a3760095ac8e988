// fsk_processor_remap_api.hip -- C ABI of libfskhip.so (include/fskhip_next.h): fskhip_processor_remap, and processor snapshots
// (fskhip_processor_snapshot_bytes / _snapshot / _snapshot_info_get / _snapshot_concat, fskhip_processor_restore).  They carry the FSKProcessor row
// -- RX rings, pending modulations, `completed` counts -- where fskhip_remap_streams and the stream snapshots carry the FSKCore
// below it.  The image's format is documented in the header; its layout and the one definition of a valid image are
// fsk_processor_image.h's (host-only, on fsk_image.h's frame: the header, the sizes and the concatenation are defined there).  Kernels:
// fsk_processor_remap.hip; the selection and room checks and the slab pipelines: fsk_stage.h, shared with the other three
// snapshot units.
#include <algorithm>
#include <vector>

#include "fsk_engine.h"
#include "fsk_launch.h"
#include "fsk_proc.h"
#include "fsk_processor_image.h"
#include "fsk_stage.h"

using namespace fsk;

namespace {

// the longest pending payload among streams idx[0 .. n) of p (idx null: all its streams; -1 entries skipped).  After the
// caller's device synchronisation; p is read only.
int max_pending_payload(const char *who, const fskhip_processor *p, const int64_t *idx, uint32_t n, uint32_t *out) {
  Scratch sc;
  int64_t *d_idx = nullptr;
  uint32_t *d_out = nullptr;
  if (const int rc = sc.alloc(d_out, 1)) return rc;
  if (idx && n)
    if (const int rc = sc.upload(d_idx, idx, n)) return rc;
  hipError_t err = launch_processor_max_payload(p->T, d_idx, idx ? n : p->S, d_out, nullptr);
  if (err == hipSuccess) err = hipMemcpy(out, d_out, sizeof(uint32_t), hipMemcpyDeviceToHost);
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
  Scratch sc;
  int64_t *d_map = nullptr;
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  HIP_TRY_AS(launch_processor_gather(dst->T, dst->S, d_map, src->T, nullptr), "proc_gather_kernel", false, (void)0);
  HIP_TRY_AS(hipDeviceSynchronize(), "hipDeviceSynchronize", false, (void)0);
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
  return proc_image_bytes(n_sel, p->T.rx_cap, (uint32_t)image_round16(max_pay));
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
  const uint32_t pay_cap = (uint32_t)image_round16(max_pay);
  const size_t rec_bytes = proc_record_bytes(p->T.rx_cap, pay_cap), need = proc_image_bytes(n_sel, p->T.rx_cap, pay_cap);
  if (const int rc = check_room(who, n_sel, need, buf, cap, written)) return rc;

  ProcHeader h = proc_image_header(n_sel, p->T.rx_cap, pay_cap);
  unsigned char *rec = (unsigned char *)buf + sizeof(ProcHeader);
  SnapSum sum;
  snap_sum(sum, &h, sizeof(h));   // (checksum field still 0)

  const auto pack = [&](const int64_t *d_sel, uint32_t first, uint32_t count, void *d_buf, hipStream_t stream) {
    const ProcImage I{nullptr, (uint32_t)rec_bytes, pay_cap, (uint32_t)image_round16(p->T.rx_cap), first, count};
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
  if (const int rc = open_image(who, proc_image_open, buf, size, &s)) return rc;
  if (!info) return fail(FSKHIP_E_INVALID, "%s: null info", who);
  std::memset(info, 0, sizeof(*info));
  info->n_streams = s.h.n_records; info->rx_capacity = s.h.rx_capacity; info->payload_capacity = s.h.payload_capacity;
  info->record_bytes = s.h.record_bytes;
  return FSKHIP_OK;
}

int fskhip_processor_snapshot_concat(const void *const *bufs, const size_t *sizes, uint32_t n, void *out, size_t cap, size_t *written) {
  static_assert(kProcConcatInvalid == FSKHIP_E_INVALID && kProcConcatOverflow == FSKHIP_E_OVERFLOW, "proc_image_concat returns the ABI's codes");
  char msg[512] = "";
  if (const int rc = proc_image_concat(bufs, sizes, n, out, cap, written, msg, sizeof(msg))) return fail(rc, "fskhip_processor_snapshot_concat: %s", msg);
  return FSKHIP_OK;
}

int fskhip_processor_restore(fskhip_processor *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_processor_restore";
  if (const int rc = remap_check_map(who, "a record of the snapshot", map, n_map)) return rc;
  ProcSnap s;
  if (const int rc = open_image(who, proc_image_open, buf, size, &s)) return rc;
  if (!dst) return fail(FSKHIP_E_INVALID, "%s: null processor", who);
  const ProcHeader &h = s.h;
  if (const int rc = check_dst(who, dst, "the snapshot", "records", h.n_records, h.rx_capacity, map, n_map)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = processor_grow_payload(dst, h.payload_capacity)) return rc;
  if (n_map == 0) return FSKHIP_OK;

  const auto unpack = [&](const int64_t *d_map, uint32_t first, uint32_t count, bool fresh_too, void *d_buf, hipStream_t stream) {
    const ProcImage I{(const uint8_t *)d_buf, h.record_bytes, h.payload_capacity, (uint32_t)image_round16(h.rx_capacity), first, count};
    return launch_processor_unpack(dst->T, dst->S, d_map, I, fresh_too, stream);
  };
  return stage_records_in(who, dst->stream, map, n_map, s.rec, h.n_records, h.record_bytes, unpack);
}

}  // extern "C"
