// fsk_history_host.h -- the history rows of the two rate converters (fsk_resample.hip, fsk_ratecvt.hip), each piece once: a handle
// keeps [S][h] floats per stream, oldest first, in the buffer its next call reads; reset zeroes one stream's row or all, state_get /
// state_set copy the rows to and from the host.  `null_text` is the unit's refusal of a null handle, `who` the entry point's name.
// Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "fsk_filter_host.h"

namespace fsk {

static __global__ void history_reset_kernel(float *hist, uint32_t h, uint32_t n_streams, int64_t stream) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n_streams * h) return;
  if (stream >= 0 && (int64_t)(idx / h) != stream) return;
  hist[idx] = 0.0f;
}

// reset: `hist` to zero for one stream, or all when stream < 0
inline int history_reset(const FilterHost *f, const char *null_text, float *hist, uint32_t h, int64_t stream) {
  if (!f) return fail(FSKHIP_E_INVALID, "%s", null_text);
  if (const int rc = filter_reset_begin(f, stream)) return rc;
  if (h) {
    const size_t total = (size_t)f->S * h;
    hipLaunchKernelGGL(history_reset_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, hist, h, f->S, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  return FSKHIP_OK;
}

// state_get (to_host) / state_set: the rows between `hist` and `state`; nothing is copied when the history is empty
inline int history_copy(const FilterHost *f, const char *null_text, const char *who, float *hist, uint32_t h, float *state, bool to_host) {
  if (!f) return fail(FSKHIP_E_INVALID, "%s", null_text);
  if (!h) return FSKHIP_OK;
  if (!state) return fail(FSKHIP_E_INVALID, "%s: null buffer", who);
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = sizeof(float) * (size_t)f->S * h;
  if (to_host) HIP_TRY(hipMemcpy(state, hist, bytes, hipMemcpyDeviceToHost));
  else HIP_TRY(hipMemcpy(hist, state, bytes, hipMemcpyHostToDevice));
  return FSKHIP_OK;
}

}  // namespace fsk
