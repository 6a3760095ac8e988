// fsk_filter_host.h -- the host part the two batched filters share (fsk_fir.hip, fsk_iir.hip), each piece once: what a handle
// holds besides its coefficients and histories, the tail of create, destroy, the front of reset, and the _host call -- rows
// through the handle's staging slabs and its _device entry point; and what the two rate converters' handles hold on top of that
// (RateHost, Slab).  Not part of the ABI.
#pragma once
#include <initializer_list>

#include "fsk_host.h"

namespace fsk {

struct FilterHost {   // (struct fskhip_fir and struct fskhip_iir derive from it)
  int device = 0;
  int precision = 0;
  uint32_t S = 0;
  hipStream_t stream = nullptr;   // the _host entry points' own
  unsigned char *d_in = nullptr, *d_out = nullptr; size_t d_in_cap = 0, d_out_cap = 0;   // their staging slabs (bytes), kept across calls
};

// what the handles of the two rate converters hold on top of it (struct fskhip_resampler and struct fskhip_ratecvt derive from
// it); their host routines are fsk_rate_host.h's
struct RateHost : FilterHost {
  int direction = 0;
  uint32_t L = 1, n_taps = 0, H = 0;      // L: the up factor (the resampler's only one); H: floats of history per stream
  double *d_taps = nullptr;               // fp64 path, in the order the unit's kernels read them
  float *d_taps32 = nullptr;              // the same, rounded once on the host (fp32 path)
  float *hist[2] = {nullptr, nullptr};    // ping-pong: [cur] is read by the next call
  int cur = 0;
  uint32_t *d_lens = nullptr;             // the _host form's per-stream lengths

  const void *taps() const { return precision == FSKHIP_PRECISION_F64 ? (const void *)d_taps : (const void *)d_taps32; }
};

// the tail of create: `err` is what the filter's own allocations, copies and memsets came to; a failed create leaves no handle
template <class F>
int filter_open(F *f, hipError_t err, const char *who, int (*destroy)(F *), F **out) {
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    destroy(f);
    return fail(err == hipErrorOutOfMemory ? FSKHIP_E_NOMEM : FSKHIP_E_HIP, "%s: %s", who, hipGetErrorString(err));
  }
  *out = f;
  return FSKHIP_OK;
}

// destroy, all but the delete: `bufs` are the filter's own device buffers
inline void filter_close(FilterHost &f, std::initializer_list<void *> bufs) {
  (void)hipSetDevice(f.device);
  (void)hipDeviceSynchronize();
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  if (f.d_in) (void)hipFree(f.d_in);
  if (f.d_out) (void)hipFree(f.d_out);
  if (f.stream) (void)hipStreamDestroy(f.stream);
}

// the front of reset (stream < 0: every stream); returns with the filter's device current and idle
inline int filter_reset_begin(const FilterHost *f, int64_t stream) {
  if (!f) return fail(FSKHIP_E_INVALID, "null filter");
  if (stream >= (int64_t)f->S) return fail(FSKHIP_E_INVALID, "stream out of range");
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

// rows x cols elements of esz bytes between the host and a device slab whose rows are padded to whole 16-byte vectors: what the
// _host calls of the rate converters (fsk_resample.hip, fsk_ratecvt.hip) stage a format's samples through
struct Slab { size_t rows, cols, esz, pitch; size_t bytes() const { return rows * pitch * esz; } };
inline Slab slab(size_t rows, size_t cols, size_t esz) { return {rows, cols, esz, (cols * esz + 15u) / 16u * 16u / esz}; }

// A _host call: S rows of n elements from `in` to the device (rows padded to whole 16-byte vectors), device(d_in, d_out, pitch,
// stream) -- the filter's _device entry point on the handle's stream --, S rows back to `out`.  Pitches in elements; the two
// texts are the entry point's refusals of a null buffer and of a pitch below n.  Synchronous.
template <typename T, class Device>
int filter_rows_host(FilterHost *f, const char *null_text, const char *pitch_text, const T *in, size_t n, size_t in_pitch, T *out,
                     size_t out_pitch, Device device) {
  if (!f) return fail(FSKHIP_E_INVALID, "null filter");
  if (n == 0) return FSKHIP_OK;
  if (!in || !out) return fail(FSKHIP_E_INVALID, "%s", null_text);
  if (in_pitch < n || out_pitch < n) return fail(FSKHIP_E_INVALID, "%s", pitch_text);
  HIP_TRY(hipSetDevice(f->device));
  constexpr size_t VN = 16 / sizeof(T);
  const size_t dp = (n + VN - 1) / VN * VN, S = f->S;
  int rc;
  if ((rc = ensure(f->d_in, f->d_in_cap, dp * S * sizeof(T))) != FSKHIP_OK) return rc;
  if ((rc = ensure(f->d_out, f->d_out_cap, dp * S * sizeof(T))) != FSKHIP_OK) return rc;
  HIP_TRY(hipMemcpy2DAsync(f->d_in, dp * sizeof(T), in, in_pitch * sizeof(T), n * sizeof(T), S, hipMemcpyHostToDevice, f->stream));
  if ((rc = device((const T *)f->d_in, (T *)f->d_out, dp, f->stream)) != FSKHIP_OK) return rc;
  HIP_TRY(hipMemcpy2DAsync(out, out_pitch * sizeof(T), f->d_out, dp * sizeof(T), n * sizeof(T), S, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  return FSKHIP_OK;
}

}  // namespace fsk
