// fsk_ratecvt.hip -- rate conversion by a ratio L / M on the device (include/fskhip_next.h: fskhip_ratecvt_*): 44.1 kHz audio in
// front of and behind an engine at 48 kHz.  The reference's FIRFilter (src/dsp/filters.ts:112-167) over the input zero-stuffed by L
// with every M-th output kept, evaluated polyphase -- neither a stuffed zero nor a dropped output is ever made.  One side is in a
// capture format and layout (fsk_samples_dev.h), the other the float32 [stream][pitch] rows of the engine.  Every output
// accumulates its products in the FIR's order (ascending tap index, `mac`), so the results are fsk_fir.hip's bit for bit; a
// skipped product with a stuffed zero can only change a zero's sign.
//
// The arithmetic of periods, rows, workgroups and LDS is fsk_ratecvt_plan.h's.  A workgroup stages the decoded inputs of its
// periods and the history in front of them in LDS, and writes the handle's next history from what it staged (each entry by the one
// workgroup that owns the sample; the two history buffers ping-pong as fskhip_resampler's do).  A lane owns the same place q of
// four periods, one per row: consecutive lanes hold consecutive outputs, so they differ in phase -- the taps lie in output order,
// [k][q], and a wave reads consecutive words of them, once for its four rows -- and their inputs x[m - k] are the same or the next
// LDS word where L > M, at most ceil(M / L) apart otherwise.  PLAYBACK in sample-major layout leaves through a [outputs][ns + 1]
// tile.
//
// One body, ratecvt_body, in two forms.  ANY lays a call of any length from any position of the handle (fsk_ratecvt_plan.h: "Calls
// of any length") on the period grid `pos` inputs in front of the call's first: it stages from there, skips the places whose
// output is not the call's and stores output j of the grid at column j - ceil(pos L / M).  !ANY is a call of whole periods from
// position 0, which owns every output of its grid and so has neither the skip nor the position (it measured 1.22 times faster for
// fp32 playback frames): both forms keep their 32 instantiations, in one table with one signature, and launch_ratecvt picks.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <vector>

#include "fsk_launch.h"
#include "fsk_mac_dev.h"
#include "fsk_rate_host.h"
#include "fsk_ratecvt.h"
#include "fsk_ratecvt_plan.h"
#include "fsk_samples_dev.h"

namespace fsk {
namespace {

struct RatecvtShape { uint32_t hist, G, rows, log2_ns, x_pitch, row_stride, span, seg_periods, split; };   // (RatecvtPlan's, as the kernels take it)

// one signature for both directions and both forms: CAPTURE reads `src` in the format and writes float rows, PLAYBACK the other
// way round; n_in = inputs per stream; d_lens is PLAYBACK's; pos: the handle's position (ANY; unused otherwise)
#define FSK_RATECVT_PARAMS                                                                                                       \
  const void *__restrict__ src_, size_t src_pitch, const uint32_t *__restrict__ d_lens, void *__restrict__ dst_, size_t dst_pitch, \
      const float *__restrict__ hist_in, float *__restrict__ hist_out, const void *__restrict__ taps_, const uint32_t *__restrict__ table, \
      uint32_t n_streams, size_t n_in, uint32_t L, uint32_t M, uint32_t n_taps, RatecvtShape G, uint32_t pos
#define FSK_RATECVT_ARGS src_, src_pitch, d_lens, dst_, dst_pitch, hist_in, hist_out, taps_, table, n_streams, n_in, L, M, n_taps, G, pos

template <typename Real, int FMT, int LAYOUT, int DIR, bool ANY>
__device__ __forceinline__ void ratecvt_body(FSK_RATECVT_PARAMS) {
  using F = SampleFmt<FMT>;
  constexpr bool kRows = LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR, kPlay = DIR == FSKHIP_RATECVT_PLAYBACK;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *const xs = reinterpret_cast<float *>(lds_raw);                 // [ns][x_pitch]: hist floats of history, then the periods' inputs
  const Real *const taps = (const Real *)taps_;                          // [K][L]
  const uint32_t tid = threadIdx.x;
  const uint32_t H = G.hist, span = G.span, ns = 1u << G.log2_ns;
  uint32_t *const tile = reinterpret_cast<uint32_t *>(xs + (size_t)ns * G.x_pitch);   // [G L][ns + 1] (PLAYBACK, sample-major)
  const uint32_t hi = blockIdx.x / G.split, lo = blockIdx.x - hi * G.split;
  const uint32_t s0 = kRows ? hi : lo << G.log2_ns;
  const size_t per0 = (size_t)(kRows ? lo : hi) * G.seg_periods;        // the workgroup's first period
  // m0, j0: the period's first input and output on the period grid, which begins `pos` inputs in front of the call (ANY; at the
  // call's first otherwise); the call's outputs are j_lo .. j_hi - 1 of the grid, those whose newest input lies in the call
  const size_t m0 = per0 * M, j0 = per0 * L;
  const size_t j_lo = ANY ? ((size_t)pos * L + M - 1u) / M : 0u, j_hi = ANY ? ((pos + n_in) * L + M - 1u) / M : n_in / M * L;

  // input i of the staged span of stream s0 + c; `len`: inputs of the call from there on read as 0.0f
  auto stage = [&](uint32_t c, uint32_t i, size_t len) {
    const uint32_t s = s0 + c;
    const int64_t m = (int64_t)m0 + (int64_t)i - (int64_t)H - (int64_t)(ANY ? pos : 0u);   // counted from the call's first input
    float v = 0.0f;
    if (s < n_streams) {
      if (m >= 0) {
        if ((size_t)m < len) {
          if constexpr (kPlay) v = ((const float *)src_)[(size_t)s * src_pitch + (size_t)m];
          else v = F::decode(((const typename F::T *)src_)[kRows ? (size_t)s * src_pitch + (size_t)m : (size_t)m * src_pitch + s]);
        }
      } else if (!ANY || m >= -(int64_t)H) {                            // (ANY: the first workgroup's `pos` words in front of the history are no input)
        v = hist_in[(size_t)s * H + (size_t)(m + (int64_t)H)];
      }
      // the history after the call: the last H samples, each written by the workgroup whose periods hold it (the first
      // workgroup's for what stays of the old history)
      const int64_t h = m + (int64_t)H - (int64_t)n_in;
      if ((i >= H || m0 == 0) && h >= 0 && m < (int64_t)n_in) hist_out[(size_t)s * H + (size_t)h] = v;
    }
    xs[c * G.x_pitch + i] = v;
  };
  if constexpr (kRows || kPlay) {                                        // the staged side lies stream by stream
    for (uint32_t c = 0; c < ns; c++) {
      size_t len = n_in;
      if (kPlay && d_lens && s0 + c < n_streams) len = d_lens[s0 + c] < n_in ? (size_t)d_lens[s0 + c] : n_in;
      for (uint32_t i = tid; i < span; i += kResampleThreads) stage(c, i, len);
    }
  } else {                                                               // frames: consecutive lanes take a frame's streams
    for (uint32_t idx = tid; idx < (span << G.log2_ns); idx += kResampleThreads) stage(idx & (ns - 1u), idx >> G.log2_ns, n_in);
  }
  __syncthreads();

  // item w: place u = w % (G L) of the rows 4 (w / (G L)) .. + 3.  Row r is block r of the stream (stream-major; output
  // j0 + r G L + u) or stream s0 + r (sample-major; output j0 + u); its inputs start r * row_stride floats into xs.
  const uint32_t Qs = G.G * L, n_quads = (G.rows + 3u) / 4u;
  const uint32_t k_full = n_taps / L, rem = n_taps - k_full * L;        // phase p has k_full + (p < rem) taps
  for (uint32_t w = tid; w < n_quads * Qs; w += kResampleThreads) {
    const uint32_t quad = w / Qs, u = w - quad * Qs;
    const uint32_t per = u / L, q = u - per * L;
    const uint32_t word = table[q], p = word >> 16;
    const uint32_t x0 = H + per * M + (word & 0xFFFFu);                  // x[m] of row 0 of the stream's span; x[m - k]: k <= H
    const auto grid_output = [&](uint32_t row) -> size_t { return j0 + (kRows ? (size_t)row * Qs : 0u) + u; };
    uint32_t xb[4];
    bool own[4];                                                         // (ANY) row r's output is the call's
    if constexpr (ANY) {
      // a place outside the call's outputs is not evaluated: the lane's first own row is computed again in its stead, unused, and
      // a lane without one has nothing to do
      uint32_t first = 4u;
#pragma unroll
      for (uint32_t r = 4u; r-- > 0u;) {
        const uint32_t row = quad * 4u + r;
        const size_t j = grid_output(row);
        own[r] = row < G.rows && j >= j_lo && j < j_hi;
        if (own[r]) first = r;
      }
      if (first == 4u) continue;
#pragma unroll
      for (uint32_t r = 0; r < 4u; r++) xb[r] = (quad * 4u + (own[r] ? r : first)) * G.row_stride + x0;
    } else {
#pragma unroll
      for (uint32_t r = 0; r < 4u; r++) {
        const uint32_t row = quad * 4u + r < G.rows ? quad * 4u + r : quad * 4u;   // (a row past the last computes the quad's first again, unused)
        xb[r] = row * G.row_stride + x0;
      }
    }
    Real acc[4] = {0, 0, 0, 0};
    const Real *tp = taps + q;
#pragma unroll 4
    for (uint32_t k = 0; k < k_full; k++) {
      const Real cc = tp[(size_t)k * L];
#pragma unroll
      for (uint32_t r = 0; r < 4u; r++) acc[r] = mac(acc[r], cc, xs[xb[r] - k]);
    }
    if (p < rem) {
      const Real cc = tp[(size_t)k_full * L];
#pragma unroll
      for (uint32_t r = 0; r < 4u; r++) acc[r] = mac(acc[r], cc, xs[xb[r] - k_full]);
    }
#pragma unroll
    for (uint32_t r = 0; r < 4u; r++) {
      const uint32_t row = quad * 4u + r;
      if (!ANY && row >= G.rows) continue;
      const size_t j = grid_output(row);
      const uint32_t s = kRows ? s0 : s0 + row;
      if ((ANY ? !own[r] : j >= j_hi) || s >= n_streams) continue;
      if constexpr (!kPlay) {
        ((float *)dst_)[(size_t)s * dst_pitch + (j - j_lo)] = (float)acc[r];
      } else if constexpr (kRows) {
        ((typename F::Bits *)dst_)[(size_t)s * dst_pitch + (j - j_lo)] = (typename F::Bits)F::encode((float)acc[r]);
      } else {
        tile[u * (ns + 1u) + row] = F::encode((float)acc[r]);
      }
    }
  }
  if constexpr (kPlay && !kRows) {
    __syncthreads();
    for (uint32_t idx = tid; idx < (Qs << G.log2_ns); idx += kResampleThreads) {
      const uint32_t c = idx & (ns - 1u), u = idx >> G.log2_ns;
      if (s0 + c < n_streams && j0 + u >= j_lo && j0 + u < j_hi)
        ((typename F::Bits *)dst_)[(j0 + u - j_lo) * dst_pitch + s0 + c] = (typename F::Bits)tile[u * (ns + 1u) + c];
    }
  }
}

#define FSK_RATECVT_KERNEL(NAME, DIR, ANY)                                                                                      \
  template <typename Real, int FMT, int LAYOUT>                                                                                 \
  __global__ __launch_bounds__(kResampleThreads) void NAME(FSK_RATECVT_PARAMS) { ratecvt_body<Real, FMT, LAYOUT, DIR, ANY>(FSK_RATECVT_ARGS); }
FSK_RATECVT_KERNEL(ratecvt_capture_kernel, FSKHIP_RATECVT_CAPTURE, false)
FSK_RATECVT_KERNEL(ratecvt_playback_kernel, FSKHIP_RATECVT_PLAYBACK, false)
FSK_RATECVT_KERNEL(ratecvt_capture_any_kernel, FSKHIP_RATECVT_CAPTURE, true)
FSK_RATECVT_KERNEL(ratecvt_playback_any_kernel, FSKHIP_RATECVT_PLAYBACK, true)

// every instantiation, once: [any][direction][precision][format][layout], in the order of the headers' enums
using RatecvtFn = void (*)(const void *, size_t, const uint32_t *, void *, size_t, const float *, float *, const void *, const uint32_t *, uint32_t, size_t, uint32_t,
                           uint32_t, uint32_t, RatecvtShape, uint32_t);
const KernelEntry<RatecvtFn> kRatecvtKernels[2][2][2][4][2] = {
    {{FSK_FORMAT_KERNELS(ratecvt_capture_kernel, float), FSK_FORMAT_KERNELS(ratecvt_capture_kernel, double)},
     {FSK_FORMAT_KERNELS(ratecvt_playback_kernel, float), FSK_FORMAT_KERNELS(ratecvt_playback_kernel, double)}},
    {{FSK_FORMAT_KERNELS(ratecvt_capture_any_kernel, float), FSK_FORMAT_KERNELS(ratecvt_capture_any_kernel, double)},
     {FSK_FORMAT_KERNELS(ratecvt_playback_any_kernel, float), FSK_FORMAT_KERNELS(ratecvt_playback_any_kernel, double)}}};

}  // namespace

hipError_t launch_ratecvt(int direction, int precision, const void *d_src, size_t src_pitch, const uint32_t *d_lens, void *d_dst, size_t dst_pitch, int format,
                          int layout, uint32_t n_streams, uint32_t pos, size_t n_in, uint32_t up, uint32_t down, uint32_t n_taps, const void *d_taps,
                          const uint32_t *d_table, const float *d_hist_in, float *d_hist_out, hipStream_t st) {
  const bool any = pos != 0 || n_in % down != 0;                         // whole periods from a boundary keep their own kernels
  const RatecvtPlan P = ratecvt_plan(layout == FSKHIP_LAYOUT_STREAM_MAJOR, direction == FSKHIP_RATECVT_PLAYBACK, up, down, n_taps, n_streams, pos, n_in);
  if (P.blocks == 0) return hipErrorInvalidValue;
  const RatecvtShape G = {P.hist, P.G, P.rows, P.log2_ns, P.x_pitch, P.row_stride, P.span, P.seg_periods, P.split};
  const KernelEntry<RatecvtFn> &k = kRatecvtKernels[any][direction][precision == FSKHIP_PRECISION_F64 ? 1 : 0][format][layout];
  hipLaunchKernelGGL(k.fn, dim3((uint32_t)P.blocks), dim3(kResampleThreads), P.lds_bytes, st, d_src, src_pitch, d_lens, d_dst, dst_pitch, d_hist_in, d_hist_out, d_taps,
                     d_table, n_streams, n_in, up, down, n_taps, G, pos);
  return hipGetLastError();
}
}  // namespace fsk

using namespace fsk;

namespace {

// The eight process entry points: `direction` is the entry point's, `host` its form, `any` whether it takes any length.  Refused
// in the header's order (fsk_rate_call.h), an n_in that is no multiple of the down factor last where the call wants one; then one
// launch from the handle's position over the buffers or the staging slabs, and the position moves on (by nothing for whole
// periods).  *n_out (may be null): what a call that was not refused wrote per stream.
int process(fskhip_ratecvt *r, const char *who, int direction, bool host, bool any, int format, int layout, size_t n_in, const void *src, size_t src_pitch,
            const uint32_t *lens, void *dst, size_t dst_pitch, size_t *n_out, hipStream_t st) {
  if (!r) return fail(FSKHIP_E_INVALID, "null rate converter");
  const uint32_t pos = r->pos;
  const size_t written = any ? ratecvt_out_count_any(r->L, r->M, pos, n_in) : ratecvt_out_count(r->L, r->M, n_in);
  const RateCall c = rate_call(r, direction, direction == FSKHIP_RATECVT_CAPTURE, format, layout, n_in, written, src, src_pitch, lens, dst, dst_pitch, any ? 1u : r->M);
  switch (const RateRefusal why = rate_call_check(c)) {
    case RateRefusal::direction:
      return fail(FSKHIP_E_INVALID, "%s: the handle converts for %s", who, r->direction == FSKHIP_RATECVT_CAPTURE ? "capture" : "playback");
    case RateRefusal::multiple: return fail(FSKHIP_E_INVALID, "%s: n_in %zu is not a multiple of the down factor %u", who, n_in, r->M);
    default:
      if (const int rc = rate_call_fail(who, format, c, why)) return rc;
  }
  const int rc = rate_process(r, c, host, direction == FSKHIP_RATECVT_CAPTURE, src, src_pitch, lens, dst, dst_pitch, st,
                              [=](const void *d_src, size_t d_src_pitch, const uint32_t *d_lens, void *d_dst, size_t d_dst_pitch, hipStream_t s) {
    return rate_run(r, [=](const float *hist_in, float *hist_out) -> int {
      const hipError_t err = launch_ratecvt(r->direction, r->precision, d_src, d_src_pitch, d_lens, d_dst, d_dst_pitch, format, layout, r->S, pos, n_in, r->L,
                                            r->M, r->n_taps, r->taps(), r->d_table, hist_in, hist_out, s);
      if (err == hipErrorInvalidValue) return rate_grid_fail(who, r->S, n_in);
      HIP_TRY(err);
      r->pos = ratecvt_next_position(r->M, pos, n_in);
      return FSKHIP_OK;
    });
  });
  if (rc == FSKHIP_OK && n_out) *n_out = written;
  return rc;
}

}  // namespace

extern "C" {

uint32_t fskhip_ratecvt_streams(const fskhip_ratecvt *r) { return rate_streams(r); }
uint32_t fskhip_ratecvt_history(const fskhip_ratecvt *r) { return rate_history(r); }
int fskhip_ratecvt_destroy(fskhip_ratecvt *r) { return rate_destroy(r, r ? r->d_table : nullptr); }
int fskhip_ratecvt_reset(fskhip_ratecvt *r, int64_t stream) {   // (one stream: the position is the handle's, and stays)
  const int rc = rate_reset(r, "null rate converter", stream);
  if (rc == FSKHIP_OK && stream < 0) r->pos = 0;
  return rc;
}
uint32_t fskhip_ratecvt_position(const fskhip_ratecvt *r) { return r ? r->pos : 0u; }
int fskhip_ratecvt_position_set(fskhip_ratecvt *r, uint32_t pos) {
  if (!r) return fail(FSKHIP_E_INVALID, "null rate converter");
  if (pos >= r->M) return fail(FSKHIP_E_INVALID, "fskhip_ratecvt_position_set: position %u is not below the down factor %u", pos, r->M);
  r->pos = pos;
  return FSKHIP_OK;
}
size_t fskhip_ratecvt_out_count_any(const fskhip_ratecvt *r, size_t n_in) { return r ? ratecvt_out_count_any(r->L, r->M, r->pos, n_in) : 0u; }
size_t fskhip_ratecvt_in_count_any(const fskhip_ratecvt *r, size_t n_out) { return r ? ratecvt_in_count_any(r->L, r->M, r->pos, n_out) : 0u; }
int fskhip_ratecvt_state_get(fskhip_ratecvt *r, float *state) { return rate_state(r, "null rate converter", "fskhip_ratecvt_state_get", state, true); }
int fskhip_ratecvt_state_set(fskhip_ratecvt *r, const float *state) {
  return rate_state(r, "null rate converter", "fskhip_ratecvt_state_set", const_cast<float *>(state), false);
}

int fskhip_ratecvt_create(int device, int direction, uint32_t up, uint32_t down, const double *taps, uint32_t n_taps, uint32_t n_streams, int precision,
                          fskhip_ratecvt **out) {
  if (!taps || !out) return fail(FSKHIP_E_INVALID, "fskhip_ratecvt_create: null taps or out");
  if (n_streams == 0 || n_taps == 0) return fail(FSKHIP_E_INVALID, "fskhip_ratecvt_create: zero n_streams or n_taps");
  if (direction != FSKHIP_RATECVT_CAPTURE && direction != FSKHIP_RATECVT_PLAYBACK) return fail(FSKHIP_E_INVALID, "fskhip_ratecvt_create: unknown direction %d", direction);
  if (up < 1 || up > kRatecvtMaxFactor || down < 1 || down > kRatecvtMaxFactor)
    return fail(FSKHIP_E_INVALID, "fskhip_ratecvt_create: ratio %u / %u outside 1..%u", up, down, kRatecvtMaxFactor);
  if (ratecvt_gcd(up, down) != 1) return fail(FSKHIP_E_INVALID, "fskhip_ratecvt_create: %u / %u is not in lowest terms", up, down);
  if (precision != FSKHIP_PRECISION_F32 && precision != FSKHIP_PRECISION_F64) return fail(FSKHIP_E_INVALID, "unknown precision %d", precision);
  if (n_taps > kResampleMaxTaps) return fail(FSKHIP_E_UNSUPPORTED, "%u taps do not fit the LDS tile (max %u)", n_taps, kResampleMaxTaps);
  if (const int rc = select_device(device)) return rc;
  fskhip_ratecvt *r = new (std::nothrow) fskhip_ratecvt();
  if (!r) return fail(FSKHIP_E_NOMEM, "out of host memory");
  r->device = device; r->precision = precision; r->S = n_streams;
  r->direction = direction; r->L = up; r->M = down; r->n_taps = n_taps; r->H = resample_history(0, up, n_taps);
  r->h_taps.assign(taps, taps + n_taps);
  // column q of the [K][L] table: the taps of phase (q M) mod L, c[p], c[p + L], ... downwards (zeros behind a short phase, never read)
  const uint32_t K = resample_phase_len(up, n_taps);
  std::vector<double> t64((size_t)K * up, 0.0);
  std::vector<uint32_t> table(up);
  for (uint32_t q = 0; q < up; q++) {
    table[q] = ratecvt_table_word(up, down, q);
    for (uint32_t k = 0, i = ratecvt_phase(up, down, q); i < n_taps; k++, i += up) t64[(size_t)k * up + q] = taps[i];
  }
  return rate_open(r, t64, table, &r->d_table, "fskhip_ratecvt_create", fskhip_ratecvt_destroy, out);
}

int fskhip_ratecvt_capture_device(fskhip_ratecvt *r, const void *d_src, int format, int layout, size_t n_in, size_t src_pitch, float *d_dst, size_t dst_pitch,
                                  void *hip_stream) {
  return process(r, "fskhip_ratecvt_capture_device", FSKHIP_RATECVT_CAPTURE, false, false, format, layout, n_in, d_src, src_pitch, nullptr, d_dst, dst_pitch, nullptr, (hipStream_t)hip_stream);
}

int fskhip_ratecvt_playback_device(fskhip_ratecvt *r, const float *d_src, size_t n_in, size_t src_pitch, const uint32_t *d_lens, void *d_dst, int format,
                                   int layout, size_t dst_pitch, void *hip_stream) {
  return process(r, "fskhip_ratecvt_playback_device", FSKHIP_RATECVT_PLAYBACK, false, false, format, layout, n_in, d_src, src_pitch, d_lens, d_dst, dst_pitch, nullptr, (hipStream_t)hip_stream);
}

int fskhip_ratecvt_capture_host(fskhip_ratecvt *r, const void *src, int format, int layout, size_t n_in, size_t src_pitch, float *dst, size_t dst_pitch) {
  return process(r, "fskhip_ratecvt_capture_host", FSKHIP_RATECVT_CAPTURE, true, false, format, layout, n_in, src, src_pitch, nullptr, dst, dst_pitch, nullptr, nullptr);
}

int fskhip_ratecvt_playback_host(fskhip_ratecvt *r, const float *src, size_t n_in, size_t src_pitch, const uint32_t *lens, void *dst, int format, int layout,
                                 size_t dst_pitch) {
  return process(r, "fskhip_ratecvt_playback_host", FSKHIP_RATECVT_PLAYBACK, true, false, format, layout, n_in, src, src_pitch, lens, dst, dst_pitch, nullptr, nullptr);
}

// the same four for calls of any length, from and to the handle's position
int fskhip_ratecvt_capture_any_device(fskhip_ratecvt *r, const void *d_src, int format, int layout, size_t n_in, size_t src_pitch, float *d_dst, size_t dst_pitch,
                                      size_t *n_out, void *hip_stream) {
  return process(r, "fskhip_ratecvt_capture_any_device", FSKHIP_RATECVT_CAPTURE, false, true, format, layout, n_in, d_src, src_pitch, nullptr, d_dst, dst_pitch, n_out,
                 (hipStream_t)hip_stream);
}

int fskhip_ratecvt_playback_any_device(fskhip_ratecvt *r, const float *d_src, size_t n_in, size_t src_pitch, const uint32_t *d_lens, void *d_dst, int format,
                                       int layout, size_t dst_pitch, size_t *n_out, void *hip_stream) {
  return process(r, "fskhip_ratecvt_playback_any_device", FSKHIP_RATECVT_PLAYBACK, false, true, format, layout, n_in, d_src, src_pitch, d_lens, d_dst, dst_pitch, n_out,
                 (hipStream_t)hip_stream);
}

int fskhip_ratecvt_capture_any_host(fskhip_ratecvt *r, const void *src, int format, int layout, size_t n_in, size_t src_pitch, float *dst, size_t dst_pitch,
                                    size_t *n_out) {
  return process(r, "fskhip_ratecvt_capture_any_host", FSKHIP_RATECVT_CAPTURE, true, true, format, layout, n_in, src, src_pitch, nullptr, dst, dst_pitch, n_out, nullptr);
}

int fskhip_ratecvt_playback_any_host(fskhip_ratecvt *r, const float *src, size_t n_in, size_t src_pitch, const uint32_t *lens, void *dst, int format, int layout,
                                     size_t dst_pitch, size_t *n_out) {
  return process(r, "fskhip_ratecvt_playback_any_host", FSKHIP_RATECVT_PLAYBACK, true, true, format, layout, n_in, src, src_pitch, lens, dst, dst_pitch, n_out, nullptr);
}

}  // extern "C"

