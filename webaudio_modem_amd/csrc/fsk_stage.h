// fsk_stage.h -- what the two image writers share (fsk_snapshot_api.hip: stream snapshots; fsk_processor_remap_api.hip: processor
// snapshots): the checksum over an image, and the staging that carries records across PCIe in slabs.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "fsk_host.h"

namespace fsk {

constexpr uint32_t kSnapSlab = 8192;           // streams per staging slab: two slabs of ~9 MB on the device, whatever the batch

// Running position-dependent sum over little-endian 64-bit words (sizes here are multiples of 8): a = sum of words, b = sum of
// the running a.  Two adds per 8 bytes -- it runs at memory speed, which a byte-wise hash of a 66 MB image would not.
struct SnapSum { uint64_t a = 0, b = 0; };
inline void snap_sum(SnapSum &s, const void *p, size_t bytes) {
  const unsigned char *c = (const unsigned char *)p;
  uint64_t a = s.a, b = s.b;
  for (size_t i = 0; i + 8 <= bytes; i += 8) {
    uint64_t w;
    std::memcpy(&w, c + i, 8);
    a += w; b += a;
  }
  s.a = a; s.b = b;
}
inline uint64_t snap_sum_value(const SnapSum &s) { return s.a * 0x9E3779B97F4A7C15ull ^ s.b; }

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

}  // namespace fsk

// a HIP call inside a slab pipeline (`who` names the entry point): on failure the device is drained before the staging goes away
#define SNAP_HIP(expr)                                                                                 \
  do {                                                                                                 \
    const hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) { (void)hipDeviceSynchronize(); return fail(FSKHIP_E_HIP, "%s: %s: %s", who, #expr, hipGetErrorString(_e)); } \
  } while (0)
