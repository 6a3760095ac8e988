// fsk_resample.hip -- integer-factor rate conversion on the device (include/fskhip_next.h: fskhip_resampler_*): the reference's
// FIRFilter (src/dsp/filters.ts:112-167) over the zero-stuffed signal (up) or with every L-th output kept (down), evaluated
// polyphase -- the stuffed zeros and the dropped outputs are never made.  The low rate side is in a capture format and layout
// (fsk_samples_dev.h), the high rate side the float32 [stream][pitch] rows the demodulators read and the modulator writes, so 8 kHz
// trunk audio crosses PCIe as it is.  Every output accumulates its products in the FIR's order (ascending tap index, `mac`), so
// the results are fsk_fir.hip's bit for bit; a skipped product with a stuffed zero can only change a zero's sign.
//
// A workgroup takes a segment of one stream (stream-major) or a tile of up to 64 streams x 64 samples (sample-major), stages the
// decoded inputs and the history in front of them in LDS, and writes the handle's next history from what it staged (each entry by
// the one workgroup that owns the sample; the two history buffers ping-pong as fskhip_fir's do).  The taps are wave-uniform and
// come in through the scalar cache.  The arithmetic of segments, tiles and LDS is fsk_resample_plan.h's.
//   up     a lane owns an INPUT m and produces its L outputs phase by phase: output mL + p = sum_k c[p + kL] x[m - k], eight
//          phases' sums in registers over four inputs read once.  A wave's 64 L outputs go through LDS and leave as 16-byte stores
//          where the destination lines up.
//   down   a lane owns four OUTPUTS.  The inputs lie in LDS by residue modulo L, so the 64 outputs of a wave read 64
//          consecutive words for every tap.  The sample-major layout leaves through a [64][streams + 1] tile.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <vector>

#include "fsk_launch.h"
#include "fsk_mac_dev.h"
#include "fsk_rate_host.h"
#include "fsk_resample_plan.h"
#include "fsk_resampler.h"
#include "fsk_samples_dev.h"

namespace fsk {
namespace {

struct ResampleShape { uint32_t hist, hist_pad, seg, log2_ns, x_pitch, q_len, split; };   // (ResamplePlan's, as the kernels take it)

// one signature for both directions: up reads `src` in the format and writes float rows, down the other way round; n = inputs
// (up) / outputs (down) per stream; d_lens is down's
#define FSK_RESAMPLE_PARAMS                                                                                                      \
  const void *__restrict__ src_, size_t src_pitch, const uint32_t *__restrict__ d_lens, void *__restrict__ dst_, size_t dst_pitch, \
      const float *__restrict__ hist_in, float *__restrict__ hist_out, const void *__restrict__ taps_, uint32_t n_streams, size_t n, \
      uint32_t L, uint32_t n_taps, ResampleShape G

template <typename Real, int FMT, int LAYOUT>
__global__ __launch_bounds__(kResampleThreads) void resample_up_kernel(FSK_RESAMPLE_PARAMS) {
  using F = SampleFmt<FMT>;
  constexpr bool kRows = LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *const os = reinterpret_cast<float *>(lds_raw);                 // [wave][64 L]: a wave's outputs in time order
  float *const xs = os + (kResampleThreads / 64u) * 64u * L;            // [ns][x_pitch]: hist floats of history, then the segment
  const typename F::T *const src = (const typename F::T *)src_;
  float *const dst = (float *)dst_;
  const Real *const taps = (const Real *)taps_;                          // [L][K], phase by phase
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t H = G.hist, seg = G.seg, ns = 1u << G.log2_ns;
  const uint32_t hi = blockIdx.x / G.split, lo = blockIdx.x - hi * G.split;
  const uint32_t s0 = kRows ? hi : lo << G.log2_ns;
  const size_t m0 = (size_t)(kRows ? lo : hi) * seg;

  for (uint32_t idx = tid; idx < ((H + seg) << G.log2_ns); idx += kResampleThreads) {
    const uint32_t c = idx & (ns - 1u), i = idx >> G.log2_ns, s = s0 + c;
    const int64_t m = (int64_t)m0 + (int64_t)i - (int64_t)H;
    float v = 0.0f;
    if (s < n_streams) {
      if (m >= 0) {
        if ((size_t)m < n) v = F::decode(src[kRows ? (size_t)s * src_pitch + (size_t)m : (size_t)m * src_pitch + s]);
      } else {
        v = hist_in[(size_t)s * H + (size_t)(m + (int64_t)H)];
      }
      // the history after the call: the last H samples, each written by the workgroup whose segment holds it (the first
      // segment's for what stays of the old history)
      const int64_t h = m + (int64_t)H - (int64_t)n;
      if ((i >= H || m0 == 0) && h >= 0 && m < (int64_t)n) hist_out[(size_t)s * H + (size_t)h] = v;
    }
    xs[c * G.x_pitch + i] = v;
  }
  __syncthreads();

  const uint32_t K = (n_taps + L - 1u) / L, k_full = n_taps / L, rem = n_taps - k_full * L;   // phase p has k_full + (p < rem) taps
  const uint32_t n_tasks = kRows ? seg >> 6 : ns;                       // rows of 64 inputs of one stream
  float *const ow = os + wave * 64u * L;
  for (uint32_t task0 = 0; task0 < n_tasks; task0 += kResampleThreads / 64u) {
    const uint32_t task = task0 + wave;
    const uint32_t c = kRows ? 0u : task, blk = kRows ? task : 0u;
    const size_t mb = m0 + (size_t)blk * 64u;                           // the row's first input
    const bool active = task < n_tasks && s0 + c < n_streams && mb < n;
    if (active) {
      const float *const xp = xs + c * G.x_pitch + H + blk * 64u + lane;   // this lane's input; xp[-k] = x[m - k], k <= K - 1 <= H
      for (uint32_t p0 = 0; p0 < L; p0 += 8u) {
        Real acc[8];
#pragma unroll
        for (uint32_t pp = 0; pp < 8u; pp++) acc[pp] = 0;
        for (uint32_t k0 = 0; k0 < K; k0 += 4u) {
          float xv[4];
#pragma unroll
          for (uint32_t kk = 0; kk < 4u; kk++) {
            xv[kk] = 0.0f;
            if (k0 + kk < K) xv[kk] = xp[-(int32_t)(k0 + kk)];
          }
#pragma unroll
          for (uint32_t pp = 0; pp < 8u; pp++) {
            const uint32_t p = p0 + pp;
            if (p < L) {
              const uint32_t kp = k_full + (p < rem ? 1u : 0u);
              const Real *const cp = taps + (size_t)p * K + k0;
              if (k0 + 4u <= kp) {
#pragma unroll
                for (uint32_t kk = 0; kk < 4u; kk++) acc[pp] = mac(acc[pp], cp[kk], xv[kk]);
              } else {
#pragma unroll
                for (uint32_t kk = 0; kk < 4u; kk++)
                  if (k0 + kk < kp) acc[pp] = mac(acc[pp], cp[kk], xv[kk]);
              }
            }
          }
        }
#pragma unroll
        for (uint32_t pp = 0; pp < 8u; pp++)
          if (p0 + pp < L) ow[lane * L + p0 + pp] = (float)acc[pp];
      }
    }
    __syncthreads();
    if (active) {
      const size_t left = n - mb;
      const uint32_t cnt = (uint32_t)(left < 64u ? left : 64u) * L;     // floats of this row that are outputs
      float *const drow = dst + (size_t)(s0 + c) * dst_pitch + mb * L;
      uint32_t head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(drow) & 15u)) & 15u) / 4u;
      head = head < cnt ? head : cnt;
      const uint32_t nv = (cnt - head) / 4u, tail0 = head + 4u * nv;
      if (lane < head) drow[lane] = ow[lane];
      if (lane >= 32u && tail0 + (lane - 32u) < cnt) drow[tail0 + (lane - 32u)] = ow[tail0 + (lane - 32u)];
      if (head == 0) {
        for (uint32_t q = lane; q < nv; q += 64u) *reinterpret_cast<float4 *>(drow + 4u * q) = *reinterpret_cast<const float4 *>(ow + 4u * q);
      } else {
        for (uint32_t q = lane; q < nv; q += 64u) {
          const float *const o = ow + head + 4u * q;
          *reinterpret_cast<float4 *>(drow + head + 4u * q) = make_float4(o[0], o[1], o[2], o[3]);
        }
      }
    }
    __syncthreads();
  }
}

template <typename Real, int FMT, int LAYOUT>
__global__ __launch_bounds__(kResampleThreads) void resample_down_kernel(FSK_RESAMPLE_PARAMS) {
  using F = SampleFmt<FMT>;
  constexpr bool kRows = LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *const xs = reinterpret_cast<float *>(lds_raw);                 // [ns][L][Q]: input tt of the workgroup at [tt % L][tt / L]
  const float *const src = (const float *)src_;
  typename F::Bits *const dst = (typename F::Bits *)dst_;
  const Real *const taps = (const Real *)taps_;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t HD = G.hist, HP = G.hist_pad, Q = G.q_len, seg = G.seg, span = G.x_pitch, ns = 1u << G.log2_ns;
  uint32_t *const tile = reinterpret_cast<uint32_t *>(xs + (size_t)ns * span);   // [64][ns + 1] (sample-major)
  const uint32_t hi = blockIdx.x / G.split, lo = blockIdx.x - hi * G.split;
  const uint32_t s0 = kRows ? hi : lo << G.log2_ns;
  const size_t k0 = (size_t)(kRows ? lo : hi) * seg;                    // the workgroup's first output
  const size_t n_in = n * L;
  const int64_t t_base = (int64_t)(k0 * L) - (int64_t)HP;               // input tt = 0

  const uint32_t step_q = kResampleThreads / L, step_r = kResampleThreads - step_q * L;
  for (uint32_t c = 0; c < ns; c++) {
    const uint32_t s = s0 + c;
    const bool s_ok = s < n_streams;
    size_t len = n_in;                                                  // inputs from here on read as 0.0f
    if (d_lens && s_ok) len = d_lens[s] < n_in ? (size_t)d_lens[s] : n_in;
    uint32_t q = tid / L, r = tid - q * L;
    for (uint32_t tt = tid; tt < span; tt += kResampleThreads) {
      const int64_t t = t_base + (int64_t)tt;
      float v = 0.0f;
      if (s_ok) {
        if (t >= 0) {
          if ((size_t)t < len) v = src[(size_t)s * src_pitch + (size_t)t];
        } else if (t >= -(int64_t)HD) {
          v = hist_in[(size_t)s * HD + (size_t)(t + (int64_t)HD)];
        }
        const int64_t h = t + (int64_t)HD - (int64_t)n_in;               // (as in the up kernel)
        if ((tt >= HP || k0 == 0) && h >= 0 && t < (int64_t)n_in) hist_out[(size_t)s * HD + (size_t)h] = v;
      }
      xs[c * span + r * Q + q] = v;
      q += step_q;
      r += step_r;
      if (r >= L) { r -= L; q++; }
    }
  }
  __syncthreads();

  // output kk of the workgroup meets tap i at input tt = kk L + (HP - i) = (kk + qe) L + re
  const uint32_t n_rows = kRows ? seg >> 6 : ns;                        // rows of 64 outputs of one stream; a wave takes four
  for (uint32_t row0 = wave * 4u; row0 < n_rows; row0 += kResampleThreads / 64u * 4u) {
    uint32_t base[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
      const uint32_t row = row0 + j < n_rows ? row0 + j : row0;           // (a row past the last computes the first again, unused)
      base[j] = (kRows ? row * 64u : row * span) + lane;
    }
    Real acc[4] = {0, 0, 0, 0};
    uint32_t re = 0, qe = HP / L;
#pragma unroll 4
    for (uint32_t i = 0; i < n_taps; i++) {
      const uint32_t off = re * Q + qe;
      const Real cc = taps[i];
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) acc[j] = mac(acc[j], cc, xs[base[j] + off]);
      if (re == 0) { re = L - 1u; qe--; } else { re--; }
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
      if (row0 + j < n_rows) {
        const uint32_t w = F::encode((float)acc[j]);
        if constexpr (kRows) {
          const size_t k = k0 + (size_t)(row0 + j) * 64u + lane;
          if (k < n) dst[(size_t)s0 * dst_pitch + k] = (typename F::Bits)w;
        } else {
          tile[lane * (ns + 1u) + row0 + j] = w;
        }
      }
    }
  }
  if constexpr (!kRows) {
    __syncthreads();
    for (uint32_t idx = tid; idx < (64u << G.log2_ns); idx += kResampleThreads) {
      const uint32_t c = idx & (ns - 1u), kk = idx >> G.log2_ns;
      if (s0 + c < n_streams && k0 + kk < n) dst[(k0 + kk) * dst_pitch + s0 + c] = (typename F::Bits)tile[kk * (ns + 1u) + c];
    }
  }
}

// every instantiation, once: [direction][precision][format][layout], in the order of the headers' enums
using ResampleFn = void (*)(const void *, size_t, const uint32_t *, void *, size_t, const float *, float *, const void *, uint32_t, size_t, uint32_t, uint32_t,
                            ResampleShape);
const KernelEntry<ResampleFn> kResampleKernels[2][2][4][2] = {
    {FSK_FORMAT_KERNELS(resample_up_kernel, float), FSK_FORMAT_KERNELS(resample_up_kernel, double)},
    {FSK_FORMAT_KERNELS(resample_down_kernel, float), FSK_FORMAT_KERNELS(resample_down_kernel, double)}};

hipError_t launch_resample(int direction, const ResamplePlan &P, int precision, int format, int layout, const void *d_src, size_t src_pitch, const uint32_t *d_lens,
                           void *d_dst, size_t dst_pitch, const float *hist_in, float *hist_out, const void *d_taps, uint32_t n_streams, size_t n, uint32_t L,
                           uint32_t n_taps, hipStream_t st) {
  if (P.blocks == 0) return hipErrorInvalidValue;
  const ResampleShape G = {P.hist, P.hist_pad, P.seg, P.log2_ns, P.x_pitch, P.q_len, P.split};
  const KernelEntry<ResampleFn> &k = kResampleKernels[direction][precision == FSKHIP_PRECISION_F64 ? 1 : 0][format][layout];
  hipLaunchKernelGGL(k.fn, dim3((uint32_t)P.blocks), dim3(kResampleThreads), P.lds_bytes, st, d_src, src_pitch, d_lens, d_dst, dst_pitch, hist_in, hist_out, d_taps,
                     n_streams, n, L, n_taps, G);
  return hipGetLastError();
}

}  // namespace

// (the caller has checked format, layout, pointers, alignments and pitches: the entry points below)
hipError_t launch_resample_up(int precision, const void *d_src, int format, int layout, uint32_t n_streams, size_t n_in, size_t src_pitch, float *d_dst,
                              size_t dst_pitch, uint32_t factor, uint32_t n_taps, const void *d_phase_taps, const float *d_hist_in, float *d_hist_out,
                              hipStream_t st) {
  if (n_streams == 0 || n_in == 0) return hipSuccess;
  const ResamplePlan P = resample_up_plan(layout == FSKHIP_LAYOUT_STREAM_MAJOR, factor, n_taps, n_streams, n_in);
  return launch_resample(FSKHIP_RESAMPLE_UP, P, precision, format, layout, d_src, src_pitch, nullptr, d_dst, dst_pitch, d_hist_in, d_hist_out, d_phase_taps,
                         n_streams, n_in, factor, n_taps, st);
}

hipError_t launch_resample_down(int precision, const float *d_src, size_t n_out, size_t src_pitch, const uint32_t *d_lens, uint32_t n_streams, void *d_dst,
                                int format, int layout, size_t dst_pitch, uint32_t factor, uint32_t n_taps, const void *d_taps, const float *d_hist_in,
                                float *d_hist_out, hipStream_t st) {
  if (n_streams == 0 || n_out == 0) return hipSuccess;
  const ResamplePlan P = resample_down_plan(layout == FSKHIP_LAYOUT_STREAM_MAJOR, factor, n_taps, n_streams, n_out);
  return launch_resample(FSKHIP_RESAMPLE_DOWN, P, precision, format, layout, d_src, src_pitch, d_lens, d_dst, dst_pitch, d_hist_in, d_hist_out, d_taps, n_streams,
                         n_out, factor, n_taps, st);
}

}  // namespace fsk

using namespace fsk;

namespace {

// The four process entry points: `direction` is the entry point's, `host` its form.  Refused in the header's order
// (fsk_rate_call.h), down's n_in that is no multiple of the factor last; then one launch over the buffers or the staging slabs.
int process(fskhip_resampler *r, const char *who, int direction, bool host, int format, int layout, size_t n_in, const void *src, size_t src_pitch,
            const uint32_t *lens, void *dst, size_t dst_pitch, hipStream_t st) {
  if (!r) return fail(FSKHIP_E_INVALID, "null resampler");
  const bool up = direction == FSKHIP_RESAMPLE_UP;
  const RateCall c = rate_call(r, direction, up, format, layout, n_in, up ? n_in * r->L : n_in / r->L, src, src_pitch, lens, dst, dst_pitch, up ? 1u : r->L);
  switch (const RateRefusal why = rate_call_check(c)) {
    case RateRefusal::direction: return fail(FSKHIP_E_INVALID, "%s: the handle resamples %s", who, r->direction == FSKHIP_RESAMPLE_UP ? "up" : "down");
    case RateRefusal::multiple: return fail(FSKHIP_E_INVALID, "%s: n_in %zu is not a multiple of the factor %u", who, n_in, r->L);
    default:
      if (const int rc = rate_call_fail(who, format, c, why)) return rc;
  }
  return rate_process(r, c, host, up, src, src_pitch, lens, dst, dst_pitch, st,
                      [=](const void *d_src, size_t d_src_pitch, const uint32_t *d_lens, void *d_dst, size_t d_dst_pitch, hipStream_t s) {
    return rate_run(r, [=](const float *hist_in, float *hist_out) -> int {
      const hipError_t err =
          up ? launch_resample_up(r->precision, d_src, format, layout, r->S, n_in, d_src_pitch, (float *)d_dst, d_dst_pitch, r->L, r->n_taps, r->taps(), hist_in, hist_out, s)
             : launch_resample_down(r->precision, (const float *)d_src, n_in / r->L, d_src_pitch, d_lens, r->S, d_dst, format, layout, d_dst_pitch, r->L, r->n_taps,
                                    r->taps(), hist_in, hist_out, s);
      if (err == hipErrorInvalidValue) return rate_grid_fail(who, r->S, n_in);
      HIP_TRY(err);
      return FSKHIP_OK;
    });
  });
}

}  // namespace

extern "C" {

uint32_t fskhip_resampler_streams(const fskhip_resampler *r) { return rate_streams(r); }
uint32_t fskhip_resampler_history(const fskhip_resampler *r) { return rate_history(r); }
int fskhip_resampler_destroy(fskhip_resampler *r) { return rate_destroy(r); }
int fskhip_resampler_reset(fskhip_resampler *r, int64_t stream) { return rate_reset(r, "null resampler", stream); }
int fskhip_resampler_state_get(fskhip_resampler *r, float *state) { return rate_state(r, "null resampler", "fskhip_resampler_state_get", state, true); }
int fskhip_resampler_state_set(fskhip_resampler *r, const float *state) {
  return rate_state(r, "null resampler", "fskhip_resampler_state_set", const_cast<float *>(state), false);
}

int fskhip_resampler_create(int device, int direction, uint32_t factor, const double *taps, uint32_t n_taps, uint32_t n_streams, int precision,
                            fskhip_resampler **out) {
  if (!taps || !out) return fail(FSKHIP_E_INVALID, "fskhip_resampler_create: null taps or out");
  if (n_streams == 0 || n_taps == 0) return fail(FSKHIP_E_INVALID, "fskhip_resampler_create: zero n_streams or n_taps");
  if (direction != FSKHIP_RESAMPLE_UP && direction != FSKHIP_RESAMPLE_DOWN) return fail(FSKHIP_E_INVALID, "fskhip_resampler_create: unknown direction %d", direction);
  if (factor < 1 || factor > kResampleMaxFactor) return fail(FSKHIP_E_INVALID, "fskhip_resampler_create: factor %u outside 1..%u", factor, kResampleMaxFactor);
  if (precision != FSKHIP_PRECISION_F32 && precision != FSKHIP_PRECISION_F64) return fail(FSKHIP_E_INVALID, "unknown precision %d", precision);
  if (n_taps > kResampleMaxTaps) return fail(FSKHIP_E_UNSUPPORTED, "%u taps do not fit the LDS tile (max %u)", n_taps, kResampleMaxTaps);
  if (const int rc = select_device(device)) return rc;
  fskhip_resampler *r = new (std::nothrow) fskhip_resampler();
  if (!r) return fail(FSKHIP_E_NOMEM, "out of host memory");
  r->device = device; r->precision = precision; r->S = n_streams;
  r->direction = direction; r->L = factor; r->n_taps = n_taps; r->H = resample_history(direction, factor, n_taps);
  r->h_taps.assign(taps, taps + n_taps);
  // up: phase p's taps c[p], c[p + L], ... side by side (the slots behind a short phase are never read)
  const uint32_t K = resample_phase_len(factor, n_taps);
  std::vector<double> t64(direction == FSKHIP_RESAMPLE_UP ? (size_t)factor * K : (size_t)n_taps, 0.0);
  for (uint32_t i = 0; i < n_taps; i++) t64[direction == FSKHIP_RESAMPLE_UP ? (size_t)(i % factor) * K + i / factor : (size_t)i] = taps[i];
  return rate_open(r, t64, {}, nullptr, "fskhip_resampler_create", fskhip_resampler_destroy, out);
}

int fskhip_resampler_up_device(fskhip_resampler *r, const void *d_src, int format, int layout, size_t n_in, size_t src_pitch, float *d_dst, size_t dst_pitch,
                               void *hip_stream) {
  return process(r, "fskhip_resampler_up_device", FSKHIP_RESAMPLE_UP, false, format, layout, n_in, d_src, src_pitch, nullptr, d_dst, dst_pitch, (hipStream_t)hip_stream);
}

int fskhip_resampler_down_device(fskhip_resampler *r, const float *d_src, size_t n_in, size_t src_pitch, const uint32_t *d_lens, void *d_dst, int format,
                                 int layout, size_t dst_pitch, void *hip_stream) {
  return process(r, "fskhip_resampler_down_device", FSKHIP_RESAMPLE_DOWN, false, format, layout, n_in, d_src, src_pitch, d_lens, d_dst, dst_pitch, (hipStream_t)hip_stream);
}

int fskhip_resampler_up_host(fskhip_resampler *r, const void *src, int format, int layout, size_t n_in, size_t src_pitch, float *dst, size_t dst_pitch) {
  return process(r, "fskhip_resampler_up_host", FSKHIP_RESAMPLE_UP, true, format, layout, n_in, src, src_pitch, nullptr, dst, dst_pitch, nullptr);
}

int fskhip_resampler_down_host(fskhip_resampler *r, const float *src, size_t n_in, size_t src_pitch, const uint32_t *lens, void *dst, int format, int layout,
                               size_t dst_pitch) {
  return process(r, "fskhip_resampler_down_host", FSKHIP_RESAMPLE_DOWN, true, format, layout, n_in, src, src_pitch, lens, dst, dst_pitch, nullptr);
}

}  // extern "C"

