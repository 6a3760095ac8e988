// fsk_resample_remap.hip -- the device half of fskhip_resampler_remap / _snapshot / _restore (include/fskhip_next.h): history rows
// of a resampler gathered through a map into another handle's rows, into an image's body, or out of one.
//
// One kernel, rs_hist_gather_kernel<FROM_IMAGE>.  A row is H floats at a pitch of H floats (H = fskhip_resampler_history(): 3 and 5
// put rows off every 16-byte grid, 16 and 96 are the 8 kHz <-> 48 kHz designs, 4 095 the longest), so the destination is one dense
// array and the work is laid out over IT: the destination is cut into 16-byte quads on its own grid, consecutive lanes take
// consecutive quads, and every store instruction of a wave is one contiguous run (1 KiB of quads; single floats only for the
// array's last, partial quad and -- from an image that crosses in several slabs -- for a quad two slabs share).  A lane's four
// floats lie in one row or straddle a boundary between rows:
//   one row, and the source row agrees with the destination modulo 16 bytes    one 16-byte load
//   otherwise (in front of and behind a row boundary, or rows that disagree)   four single-float loads, each through its own
//                                                                              row's map entry
// Either way a source row is read as one contiguous run by the lanes that cover it.  A lane moves four quads 256 quads apart, all
// loads before the first store.  Map entries are re-read by the lanes that share a row (a broadcast within the wave).  Pure data
// movement: no LDS, no atomics, nothing the order of workgroups could change; words move as integers, so NaN payloads and the sign
// of zero cannot change.
//
// FROM_IMAGE: `src` is one staging slab of an image's rows, records [first, first + count); the launch covers all of the
// destination and writes the floats whose record is in the slab -- and the rows of new streams (-1) where fresh_too, which is the
// first launch's.  Otherwise every float is written: from row map[i] of `src`, or zeros for -1.  A null map is the identity
// shifted by ident0 (a snapshot of all streams packs rows ident0 .. of the handle).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_launch.h"

namespace fsk {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kInFlight = 4;   // quads per lane, loaded before the first store

// the division of a flat float index by the row length: 32-bit where the array allows it (a 64-bit one costs more than the copy)
__device__ __forceinline__ void row_of(uint64_t f, uint32_t H, bool narrow, uint64_t &row, uint32_t &col) {
  if (narrow) {
    const uint32_t r = (uint32_t)f / H;
    row = r; col = (uint32_t)f - r * H;
  } else {
    row = f / H; col = (uint32_t)(f - row * H);
  }
}

template <bool FROM_IMAGE>
__global__ __launch_bounds__(kThreads) void rs_hist_gather_kernel(uint32_t *__restrict__ dst, uint64_t n_floats, uint32_t H, const int64_t *__restrict__ map,
                                                                  int64_t ident0, const uint32_t *__restrict__ src, int64_t first, int64_t count,
                                                                  uint32_t fresh_too) {
  const bool narrow = n_floats <= 0xFFFFFFFFull;
  const uint64_t n_quads = (n_floats + 3u) >> 2;
  const uint64_t q0 = (uint64_t)blockIdx.x * (kThreads * kInFlight) + threadIdx.x;
  uint32_t w[kInFlight][4];
  uint32_t live[kInFlight];   // bit k: float k of the quad is written by this launch
#pragma unroll
  for (uint32_t u = 0; u < kInFlight; u++) {
    const uint64_t q = q0 + (uint64_t)u * kThreads;
    live[u] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) w[u][k] = 0u;
    if (q >= n_quads) continue;
    const uint64_t f = q << 2;
    uint64_t row;
    uint32_t col;
    row_of(f, H, narrow, row, col);
    if (col + 4u <= H && f + 4u <= n_floats) {   // one row holds the quad
      const int64_t m = map ? map[row] : ident0 + (int64_t)row;
      const bool fresh = m < 0, here = !FROM_IMAGE || (m >= first && m < first + count);
      if (fresh ? (!FROM_IMAGE || fresh_too != 0u) : here) live[u] = 15u;
      if (!fresh && here) {
        const uint64_t s = (uint64_t)(m - (FROM_IMAGE ? first : 0)) * H + col;   // (both bases are 16-byte aligned)
        if ((s & 3u) == 0u) {
          const uint4 v = *reinterpret_cast<const uint4 *>(src + s);
          w[u][0] = v.x; w[u][1] = v.y; w[u][2] = v.z; w[u][3] = v.w;
        } else {
#pragma unroll
          for (uint32_t k = 0; k < 4u; k++) w[u][k] = src[s + k];
        }
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) {
        if (f + k < n_floats) {
          const int64_t m = map ? map[row] : ident0 + (int64_t)row;
          const bool fresh = m < 0, here = !FROM_IMAGE || (m >= first && m < first + count);
          if (fresh ? (!FROM_IMAGE || fresh_too != 0u) : here) live[u] |= 1u << k;
          if (!fresh && here) w[u][k] = src[(uint64_t)(m - (FROM_IMAGE ? first : 0)) * H + col];
        }
        if (++col == H) { col = 0; row++; }
      }
    }
  }
#pragma unroll
  for (uint32_t u = 0; u < kInFlight; u++) {
    const uint64_t f = (q0 + (uint64_t)u * kThreads) << 2;
    if (live[u] == 15u) {
      *reinterpret_cast<uint4 *>(dst + f) = make_uint4(w[u][0], w[u][1], w[u][2], w[u][3]);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++)
        if (live[u] & (1u << k)) dst[f + k] = w[u][k];
    }
  }
}

}  // namespace

// (the caller has checked the map against the source and that both bases are 16-byte aligned; n_rows * H > 0)
hipError_t launch_resampler_hist_gather(float *d_dst, uint64_t n_rows, uint32_t H, const int64_t *d_map, int64_t ident0, const float *d_src, bool from_image,
                                        int64_t first, int64_t count, bool fresh_too, hipStream_t st) {
  const uint64_t n_floats = n_rows * H;
  if (n_floats == 0) return hipSuccess;
  const uint64_t per_block = (uint64_t)kThreads * kInFlight * 4u, blocks = (n_floats + per_block - 1) / per_block;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (from_image)
    hipLaunchKernelGGL(rs_hist_gather_kernel<true>, dim3((uint32_t)blocks), dim3(kThreads), 0, st, (uint32_t *)d_dst, n_floats, H, d_map, ident0,
                       (const uint32_t *)d_src, first, count, fresh_too ? 1u : 0u);
  else
    hipLaunchKernelGGL(rs_hist_gather_kernel<false>, dim3((uint32_t)blocks), dim3(kThreads), 0, st, (uint32_t *)d_dst, n_floats, H, d_map, ident0,
                       (const uint32_t *)d_src, (int64_t)0, (int64_t)0, 0u);
  return hipGetLastError();
}

}  // namespace fsk
