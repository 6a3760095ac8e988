// fsk_stage.h -- what the snapshot units (fsk_snapshot_api.hip, fsk_processor_remap_api.hip, fsk_xmodem_remap_api.hip, and
// fsk_rate_remap_host.h for fsk_resample_remap_api.hip and fsk_ratecvt_remap_api.hip) share that needs a device, each once: the writers' selection and room checks, and the two slab
// pipelines that carry records across PCIe -- stage_records_out for the writers, stage_records_in for the restores; no event chain is
// spelled anywhere else.  (The frame of an image is host-only: fsk_image.h, under the fsk_*_image.h.)  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "fsk_host.h"

namespace fsk {

constexpr uint32_t kSnapSlab = 8192;           // streams per staging slab: two slabs of ~9 MB on the device, whatever the batch

// two staging buffers on the device, a copy stream beside the owner's own, and the events that chain slab k's copy and kernel
struct Stage {
  void *buf[2] = {nullptr, nullptr};
  int64_t *d_idx = nullptr;
  hipStream_t copy = nullptr;
  hipEvent_t ev_kernel[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
  hipError_t open(size_t slab_bytes, const int64_t *idx, size_t n_idx) {
    hipError_t err = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking);
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
      err = hipMalloc(&buf[i], std::max<size_t>(slab_bytes, 16));
      if (err == hipSuccess) err = hipEventCreateWithFlags(&ev_kernel[i], hipEventDisableTiming);
      if (err == hipSuccess) err = hipEventCreateWithFlags(&ev_copy[i], hipEventDisableTiming);
    }
    if (err == hipSuccess && idx && n_idx) {
      err = hipMalloc((void **)&d_idx, sizeof(int64_t) * n_idx);
      if (err == hipSuccess) err = hipMemcpy(d_idx, idx, sizeof(int64_t) * n_idx, hipMemcpyHostToDevice);
    }
    return err;
  }
  ~Stage() {
    if (copy) (void)hipStreamSynchronize(copy);
    for (int i = 0; i < 2; i++) {
      if (buf[i]) (void)hipFree(buf[i]);
      if (ev_kernel[i]) (void)hipEventDestroy(ev_kernel[i]);
      if (ev_copy[i]) (void)hipEventDestroy(ev_copy[i]);
    }
    if (d_idx) (void)hipFree(d_idx);
    if (copy) (void)hipStreamDestroy(copy);
  }
};

// what the writers ask of a selection (`noun`: "engine" / "processor", which has n_streams) ...
inline int check_sel(const char *who, const char *noun, const int64_t *sel, uint32_t n_sel, uint32_t n_streams) {
  for (uint32_t i = 0; sel && i < n_sel; i++)
    if (sel[i] < 0 || sel[i] >= (int64_t)n_streams) return fail(FSKHIP_E_INVALID, "%s: sel[%u] = %lld, the %s has %u streams", who, i, (long long)sel[i], noun, n_streams);
  return FSKHIP_OK;
}
// ... and of the caller's buffer: *written is the size needed, whether or not the image fits
inline int check_room(const char *who, uint32_t n_sel, size_t need, const void *buf, size_t cap, size_t *written) {
  if (written) *written = need;
  if (!buf || cap < need) return fail(FSKHIP_E_OVERFLOW, "%s: a snapshot of %u streams takes %zu bytes, the buffer has %zu", who, n_sel, need, buf ? cap : (size_t)0);
  return FSKHIP_OK;
}

}  // namespace fsk

// a HIP call inside a slab pipeline (`who` names the entry point): on failure the device is drained before the staging goes away
#define SNAP_HIP(expr)                                                                                 \
  do {                                                                                                 \
    const hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) { (void)hipDeviceSynchronize(); return fail(FSKHIP_E_HIP, "%s: %s: %s", who, #expr, hipGetErrorString(_e)); } \
  } while (0)

namespace fsk {

// ---- the slab pipelines.  Both own the Stage, the slab size and the event chain; a format brings its launches as callables
// that return hipError_t.  `stream` is the owner's (the engine's, the processor's); the copies run on Stage::copy beside it.

// Records out: records [0, n) of rec_bytes each -- record r being row idx[r] of the owner, or row r where idx is null -- to the
// host at `rec`.  Slab k: pack(d_idx, first, count, d_buf, stream) on the owner's stream, then its copy on the copy stream;
// finish(first_record, end_record) is the host's part for a slab that has arrived, run for slab k - 1 while slab k is on its way.
template <class Pack, class Finish>
int stage_records_out(const char *who, hipStream_t stream, const int64_t *idx, uint32_t n, size_t rec_bytes, unsigned char *rec, Pack pack, Finish finish) {
  Stage st;
  const uint32_t slab = std::min<uint32_t>(kSnapSlab, std::max<uint32_t>(n, 1u));
  SNAP_HIP(st.open((size_t)slab * rec_bytes, idx, idx ? n : 0));
  const uint32_t n_slabs = (n + slab - 1) / slab;
  auto arrived = [&](uint32_t k) { finish(k * slab, std::min(n, k * slab + slab)); };
  for (uint32_t k = 0; k < n_slabs; k++) {
    const int b = (int)(k & 1u);
    const uint32_t first = k * slab, count = std::min(n - first, slab);
    if (k >= 2) SNAP_HIP(hipStreamWaitEvent(stream, st.ev_copy[b], 0));   // buffer b is free once slab k - 2 has left it
    SNAP_HIP(pack(st.d_idx, first, count, st.buf[b], stream));
    SNAP_HIP(hipEventRecord(st.ev_kernel[b], stream));
    SNAP_HIP(hipStreamWaitEvent(st.copy, st.ev_kernel[b], 0));
    SNAP_HIP(hipMemcpyAsync(rec + (size_t)first * rec_bytes, st.buf[b], (size_t)count * rec_bytes, hipMemcpyDeviceToHost, st.copy));
    SNAP_HIP(hipEventRecord(st.ev_copy[b], st.copy));
    if (k >= 1) { SNAP_HIP(hipEventSynchronize(st.ev_copy[b ^ 1])); arrived(k - 1); }
  }
  if (n_slabs) { SNAP_HIP(hipEventSynchronize(st.ev_copy[(n_slabs - 1) & 1u])); arrived(n_slabs - 1); }
  return FSKHIP_OK;
}

// Records in: the n records at `rec` to the device, for a destination whose row i takes record map[i] (-1: a fresh row).  Slab k
// crosses on the copy stream while slab k - 1 is unpacked on the owner's: unpack(d_map, first, count, fresh_too, d_buf, stream)
// covers all of the destination and serves the rows whose record is in [first, first + count) -- and the fresh rows where
// fresh_too, which is the first launch; there is a first launch even for no records.  Returns with the device idle.
template <class Unpack>
int stage_records_in(const char *who, hipStream_t stream, const int64_t *map, uint32_t n_map, const unsigned char *rec, uint32_t n, size_t rec_bytes, Unpack unpack) {
  Stage st;
  const uint32_t slab = std::min<uint32_t>(kSnapSlab, std::max<uint32_t>(n, 1u));
  SNAP_HIP(st.open((size_t)slab * rec_bytes, map, n_map));
  const uint32_t n_slabs = std::max<uint32_t>(1u, (n + slab - 1) / slab);
  for (uint32_t k = 0; k < n_slabs; k++) {
    const int b = (int)(k & 1u);
    const uint32_t first = k * slab, count = n > first ? std::min(n - first, slab) : 0u;
    if (count) {
      if (k >= 2) SNAP_HIP(hipStreamWaitEvent(st.copy, st.ev_kernel[b], 0));   // buffer b is free once slab k - 2 is unpacked
      SNAP_HIP(hipMemcpyAsync(st.buf[b], rec + (size_t)first * rec_bytes, (size_t)count * rec_bytes, hipMemcpyHostToDevice, st.copy));
      SNAP_HIP(hipEventRecord(st.ev_copy[b], st.copy));
      SNAP_HIP(hipStreamWaitEvent(stream, st.ev_copy[b], 0));
    }
    SNAP_HIP(unpack(st.d_idx, first, count, k == 0, st.buf[b], stream));
    SNAP_HIP(hipEventRecord(st.ev_kernel[b], stream));
  }
  SNAP_HIP(hipStreamSynchronize(stream));
  SNAP_HIP(hipDeviceSynchronize());
  return FSKHIP_OK;
}

}  // namespace fsk
