// fsk_remap.hip -- fskhip_remap_streams (include/fskhip.h): stream i of one engine continues stream map[i] of another, or
// starts as a new FSKCore() + configure() where map[i] = -1.  The whole per-stream state is gathered in one launch, one lane
// per destination stream:
//   - every RF_* row (Real) and IF_* row (u32), [field][stream];
//   - the polyphase sync registers, [n_blocks][d][64] -- block = stream / 64 for every kernel, the narrow groups (blk_lanes
//     32 / 16 / 8) included -- 32- or 64-bit per P.wide, and their `undefined` masks poly_u (fractional capacities);
//   - the amplitude ring, [amp_cap / 4][stream] quads of four slots (fsk_dev.h amp_index): one 16-byte load and store per
//     lane and quad.
// Stores walk the destination in its own order (coalesced); loads are gathers that coalesce wherever runs of consecutive
// map values do.  coef / nco_inc are the destination's own (its configs equal the source's, the host checked); blk_stash,
// blk_q, cu_ctr, blk_stat are per-launch scratch, not state.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_dev.h"
#include "fsk_newstream.h"
#include "fsk_params.h"
#include "fsk_launch.h"

namespace fsk {

namespace {

template <typename Real>
__global__ __launch_bounds__(256) void remap_kernel(RemapArgs A, const int64_t *__restrict__ map, DemodState D, DemodState S) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_dst) return;
  const int64_t mi = map[i];
  const bool cont = mi >= 0;
  const uint32_t m = cont ? (uint32_t)mi : 0u;
  const size_t nd = A.n_dst, ns = A.n_src;

  // ---- state words.  A new stream: fsk_newstream.h -- configure()'s values, its ring positions on the engine's grid when the
  // engine stays in lock step (the source's row 0: every stream's, in lock step), and on fp32 engines of one shared
  // configuration the free-running I/Q frame of a continued stream's source row, A.frame_row, whose config is dst's.
  // Eight loads in flight per lane before their stores (a batch of 65 536 streams is one wave per SIMD: latency-bound)
  const Real *__restrict__ srs = (const Real *)S.rs;
  Real *__restrict__ drs = (Real *)D.rs;
  const uint32_t *__restrict__ sis = S.is;
  uint32_t *__restrict__ dis = D.is;
  NewStream NS{};
  NS.matched_zero = A.matched_zero; NS.grid = A.grid_src; NS.frame = A.frame_src;
  if (!cont && A.grid_src) { NS.poly_phase = sis[(size_t)IF_poly_phase * ns]; NS.amp_pos = sis[(size_t)IF_amp_pos * ns]; }
  if (!cont && A.frame_src) {
    const size_t r = A.frame_row;
    NS.fr0 = frame_phase(sis[(size_t)IF_nco_lo * ns + r], sis[(size_t)IF_nco_hi * ns + r], sis[(size_t)IF_fr_lo * ns + r], sis[(size_t)IF_fr_hi * ns + r]);
  }
  for (int f0 = 0; f0 < RF_COUNT; f0 += 8) {
    Real v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int f = f0 + k;
      const Real x = f < RF_COUNT ? srs[(size_t)f * ns + m] : (Real)0;   // (loaded for a new stream too: m = 0, in range)
      v[k] = cont ? x : new_stream_real<Real>(f, NS);
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (f0 + k < RF_COUNT) drs[(size_t)(f0 + k) * nd + i] = v[k];
  }
  for (int f0 = 0; f0 < IF_COUNT; f0 += 8) {
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int f = f0 + k;
      const uint32_t x = f < IF_COUNT ? sis[(size_t)f * ns + m] : 0u;
      v[k] = cont ? x : new_stream_int(f, NS);
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (f0 + k < IF_COUNT) dis[(size_t)(f0 + k) * nd + i] = v[k];
  }

  // ---- polyphase sync registers (and the `undefined` masks of fractional capacities)
  const size_t dpo = (size_t)(i >> 6) * A.d * 64u + (i & 63u), spo = (size_t)(m >> 6) * A.d * 64u + (m & 63u);
  if (A.wide) {
    const uint64_t *__restrict__ sp = (const uint64_t *)S.poly;
    uint64_t *__restrict__ dp = (uint64_t *)D.poly;
    for (uint32_t p = 0; p < A.d; p++) { const uint64_t x = sp[spo + (size_t)p * 64u]; dp[dpo + (size_t)p * 64u] = cont ? x : 0ull; }
    if (A.frac) {
      const uint64_t *__restrict__ su = (const uint64_t *)S.poly_u;
      uint64_t *__restrict__ du = (uint64_t *)D.poly_u;
      for (uint32_t p = 0; p < A.d; p++) { const uint64_t x = su[spo + (size_t)p * 64u]; du[dpo + (size_t)p * 64u] = cont ? x : 0ull; }
    }
  } else {
    const uint32_t *__restrict__ sp = (const uint32_t *)S.poly;
    uint32_t *__restrict__ dp = (uint32_t *)D.poly;
    for (uint32_t p = 0; p < A.d; p++) { const uint32_t x = sp[spo + (size_t)p * 64u]; dp[dpo + (size_t)p * 64u] = cont ? x : 0u; }
  }

  // ---- amplitude ring: quad q of a stream holds slots 4q .. 4q+3
  const v4f *__restrict__ sa = (const v4f *)S.amp_ring;
  v4f *__restrict__ da = (v4f *)D.amp_ring;
  const v4f z = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t q = 0; q < (A.amp_cap >> 2); q++) { const v4f x = sa[(size_t)q * ns + m]; da[(size_t)q * nd + i] = cont ? x : z; }
}

}  // namespace

hipError_t launch_remap(int precision, const RemapArgs &A, const int64_t *d_map, const DemodState &D, const DemodState &S,
                        hipStream_t st) {
  const dim3 g((A.n_dst + 255u) / 256u), b(256);
  if (precision == 1) hipLaunchKernelGGL(remap_kernel<double>, g, b, 0, st, A, d_map, D, S);
  else hipLaunchKernelGGL(remap_kernel<float>, g, b, 0, st, A, d_map, D, S);
  return hipGetLastError();
}

}  // namespace fsk
