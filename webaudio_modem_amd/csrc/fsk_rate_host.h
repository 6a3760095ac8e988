// fsk_rate_host.h -- the host part the two rate converters share (fsk_resample.hip, fsk_ratecvt.hip) over their handles' common
// base (RateHost, fsk_filter_host.h), each piece once: the tail of create, destroy, the history rows -- [S][H] floats per stream,
// oldest first, in the buffer the next call reads: reset zeroes one stream's row or all, state_get / state_set copy the rows to
// and from the host --, the texts of a refused call (fsk_rate_call.h decides which), and a process call behind its check: device
// buffers as they are, host buffers through the handle's staging slabs.  `null_text` is the unit's refusal of a null handle,
// `who` the entry point's name.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "fsk_filter_host.h"
#include "fsk_launch.h"
#include "fsk_rate_call.h"

namespace fsk {

static __global__ void history_reset_kernel(float *hist, uint32_t h, uint32_t n_streams, int64_t stream) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n_streams * h) return;
  if (stream >= 0 && (int64_t)(idx / h) != stream) return;
  hist[idx] = 0.0f;
}

// reset: the history to zero for one stream, or all when stream < 0
inline int rate_reset(RateHost *r, const char *null_text, int64_t stream) {
  if (!r) return fail(FSKHIP_E_INVALID, "%s", null_text);
  if (const int rc = filter_reset_begin(r, stream)) return rc;
  if (r->H) {
    const size_t total = (size_t)r->S * r->H;
    hipLaunchKernelGGL(history_reset_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, r->hist[r->cur], r->H, r->S, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  return FSKHIP_OK;
}

// state_get (to_host) / state_set: the rows between the history and `state`; nothing is copied when the history is empty
inline int rate_state(RateHost *r, const char *null_text, const char *who, float *state, bool to_host) {
  if (!r) return fail(FSKHIP_E_INVALID, "%s", null_text);
  if (!r->H) return FSKHIP_OK;
  if (!state) return fail(FSKHIP_E_INVALID, "%s: null buffer", who);
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = sizeof(float) * (size_t)r->S * r->H;
  if (to_host) HIP_TRY(hipMemcpy(state, r->hist[r->cur], bytes, hipMemcpyDeviceToHost));
  else HIP_TRY(hipMemcpy(r->hist[r->cur], state, bytes, hipMemcpyHostToDevice));
  return FSKHIP_OK;
}

inline uint32_t rate_streams(const RateHost *r) { return r ? r->S : 0u; }
inline uint32_t rate_history(const RateHost *r) { return r ? r->H : 0u; }

// destroy; `extra`: a device buffer of the unit's own
template <class R>
int rate_destroy(R *r, void *extra = nullptr) {
  if (!r) return FSKHIP_OK;
  filter_close(*r, {r->d_taps, r->d_taps32, extra, r->hist[0], r->hist[1], r->d_lens});
  delete r;
  return FSKHIP_OK;
}

// The tail of create, for a handle whose members are set: t64 are the taps in device order; `table` (may be empty) goes to a
// device buffer of the unit's own, *d_table.  The histories start as zeros.  A failed create leaves no handle.
template <class R>
int rate_open(R *r, const std::vector<double> &t64, const std::vector<uint32_t> &table, uint32_t **d_table, const char *who, int (*destroy)(R *), R **out) {
  const std::vector<float> t32(t64.begin(), t64.end());
  const size_t hsz = sizeof(float) * (size_t)r->S * (r->H ? r->H : 1u);
  hipError_t err = hipSuccess;
  const auto alloc = [&err](auto **p, size_t bytes) { if (err == hipSuccess) err = hipMalloc((void **)p, bytes); };
  const auto upload = [&err, &alloc](auto **p, const auto &host) {
    alloc(p, sizeof(host[0]) * host.size());
    if (err == hipSuccess) err = hipMemcpy(*p, host.data(), sizeof(host[0]) * host.size(), hipMemcpyHostToDevice);
  };
  upload(&r->d_taps, t64);
  upload(&r->d_taps32, t32);
  if (!table.empty()) upload(d_table, table);
  for (float *&h : r->hist) {
    alloc(&h, hsz);
    if (err == hipSuccess) err = hipMemset(h, 0, hsz);
  }
  alloc(&r->d_lens, sizeof(uint32_t) * r->S);
  return filter_open(r, err, who, destroy, out);
}

// what a refused call returns, for all that the two units word alike (FSKHIP_OK for none); the format and the layout are
// check_sample_format's, the direction and the multiple the unit's own
inline int rate_call_fail(const char *who, int format, const RateCall &c, RateRefusal why) {
  switch (why) {
    case RateRefusal::format:
    case RateRefusal::layout: return check_sample_format(who, format, c.layout);
    case RateRefusal::null_buffer: return fail(FSKHIP_E_INVALID, "%s: null buffer", who);
    case RateRefusal::float_pitch: return fail(FSKHIP_E_INVALID, "%s: float pitch %zu < %zu samples per stream", who, c.wide_pitch, c.n_wide);
    case RateRefusal::sample_pitch: return fail(FSKHIP_E_INVALID, "%s: sample pitch %zu < %zu samples per stream", who, c.narrow_pitch, c.n_narrow);
    case RateRefusal::frame_pitch: return fail(FSKHIP_E_INVALID, "%s: frame pitch %zu < n_streams %u", who, c.narrow_pitch, c.n_streams);
    case RateRefusal::alignment: return fail(FSKHIP_E_INVALID, "%s: a buffer is not aligned to its element size", who);
    default: return FSKHIP_OK;
  }
}
// a call of direction `direction` that reads n_in elements per stream at `src` and writes n_out at `dst`, as rate_call_check takes it
inline RateCall rate_call(const RateHost *r, int direction, bool narrow_in, int format, int layout, size_t n_in, size_t n_out, const void *src, size_t src_pitch,
                          const uint32_t *lens, const void *dst, size_t dst_pitch, size_t multiple) {
  const auto u = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
  return {n_in, narrow_in ? n_in : n_out, narrow_in ? n_out : n_in, r->S, u(narrow_in ? src : dst), u(narrow_in ? dst : src), u(lens),
          narrow_in ? src_pitch : dst_pitch, narrow_in ? dst_pitch : src_pitch, sample_bytes(format), layout, multiple, r->direction == direction};
}
inline int rate_grid_fail(const char *who, uint32_t n_streams, size_t n) {
  return fail(FSKHIP_E_INVALID, "%s: %u streams x %zu samples are more workgroups than one launch takes", who, n_streams, n);
}

// one launch between the handle's two histories, launch(hist_in, hist_out); they change places behind it
template <class Launch>
int rate_run(RateHost *r, Launch launch) {
  if (const int rc = launch((const float *)r->hist[r->cur], r->hist[r->cur ^ 1])) return rc;
  if (r->H) r->cur ^= 1;
  return FSKHIP_OK;
}

// A checked call `c` that reads `src` -- the narrow side where narrow_in, else the float rows -- and writes `dst`: nothing for an
// empty call; device buffers go to run(d_src, src_pitch, d_lens, d_dst, dst_pitch, stream) as they are, on `st`; host buffers
// (`host`) go through the handle's staging slabs, rows padded to whole 16-byte vectors, on its own stream, synchronously.
template <class Run>
int rate_process(RateHost *r, const RateCall &c, bool host, bool narrow_in, const void *src, size_t src_pitch, const uint32_t *lens, void *dst, size_t dst_pitch,
                 hipStream_t st, Run run) {
  if (c.n_in == 0) return FSKHIP_OK;
  HIP_TRY(hipSetDevice(r->device));
  if (!host) return run(src, src_pitch, lens, dst, dst_pitch, st);
  const bool rows = c.layout == FSKHIP_LAYOUT_STREAM_MAJOR;
  const Slab narrow = slab(rows ? r->S : c.n_narrow, rows ? c.n_narrow : r->S, c.esz), wide = slab(r->S, c.n_wide, sizeof(float));
  const Slab &in = narrow_in ? narrow : wide, &out = narrow_in ? wide : narrow;
  int rc;
  if ((rc = ensure(r->d_in, r->d_in_cap, in.bytes())) != FSKHIP_OK) return rc;
  if ((rc = ensure(r->d_out, r->d_out_cap, out.bytes())) != FSKHIP_OK) return rc;
  HIP_TRY(hipMemcpy2DAsync(r->d_in, in.pitch * in.esz, src, src_pitch * in.esz, in.cols * in.esz, in.rows, hipMemcpyHostToDevice, r->stream));
  if (lens) HIP_TRY(hipMemcpyAsync(r->d_lens, lens, sizeof(uint32_t) * r->S, hipMemcpyHostToDevice, r->stream));
  if ((rc = run(r->d_in, in.pitch, lens ? r->d_lens : nullptr, r->d_out, out.pitch, r->stream)) != FSKHIP_OK) return rc;
  if (out.rows && out.cols)   // (a call may write nothing and still move the handle on: fskhip_ratecvt_*_any_host)
    HIP_TRY(hipMemcpy2DAsync(dst, dst_pitch * out.esz, r->d_out, out.pitch * out.esz, out.cols * out.esz, out.rows, hipMemcpyDeviceToHost, r->stream));
  HIP_TRY(hipStreamSynchronize(r->stream));
  return FSKHIP_OK;
}

}  // namespace fsk
