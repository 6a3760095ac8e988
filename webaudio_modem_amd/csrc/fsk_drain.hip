// fsk_drain.hip -- the device half of fskhip_processor_rx_drain_sparse_host / _device (include/fskhip_next.h): the RX rings
// that hold bytes, compacted into a list of stream indices, CSR offsets and one tightly packed run of bytes, in stream order.
//
// Three launches, no atomics -- every position is a prefix sum, so the result is deterministic:
//   count  one lane per stream, 256 streams per workgroup: reads rx_len (and the mask), decides the selection, and reduces the
//          workgroup to one pair {selected streams, selected bytes} (ballot + popcount; a wave prefix sum; LDS across the waves).
//   scan   one workgroup turns the pairs into exclusive positions in place, 256 pairs per pass (262 144 streams: 4 passes), and
//          writes the totals {n_active, n_bytes, fits the caps}.
//   pack   the same workgroups redo their in-group scan from the same rx_len words (the code is shared: pick_and_scan), write
//          their streams[] / offsets[] entries, move the bytes and advance the selected rings.  It reads the totals first and
//          stands down as a whole when they exceed the caps: an overflowing call changes nothing.
// The bytes move the way proc_gather_kernel (fsk_processor_remap.hip) moves its rows: a wave lists the rings of its 64 streams
// that are selected, compacted through LDS, and walks them with consecutive lanes on consecutive bytes of ONE ring -- lanes per
// ring = the wave's longest span rounded up to a power of two, at most 64, so a wave of 3-byte spans moves 16 of them per pass --,
// four passes' loads issued before the first store.  A span [readIndex, readIndex + _length) that runs over the ring's end
// continues at its start.  Byte-granular on purpose: spans are a few bytes to a few hundred, with arbitrary source and
// destination alignment, and the call is expected to be bound by the pass over the length words and by launch latency.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_launch.h"
#include "fsk_params.h"
#include "fsk_pick_dev.h"

namespace fsk {

namespace {

constexpr uint32_t kInFlight = 4;   // ring passes whose loads are issued before the first store

// the drain's selection -- mask[s] and at least max(min_len, 1) bytes -- and byte count -- the whole ring content -- through the
// shared in-workgroup scan (fsk_pick_dev.h)
__device__ __forceinline__ Pick pick_and_scan(const uint32_t *__restrict__ rx_len, const uint8_t *__restrict__ mask, uint32_t n_streams, uint32_t min_len,
                                              uint32_t (*ws)[2]) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t len = s < n_streams ? rx_len[s] : 0u;
  return pick_scan(s < n_streams && len >= max(min_len, 1u) && (!mask || mask[s] != 0), len, ws);
}

__global__ __launch_bounds__(256) void drain_count_kernel(const uint32_t *__restrict__ rx_len, const uint8_t *__restrict__ mask, uint32_t n_streams,
                                                          uint32_t min_len, uint2 *__restrict__ pairs) {
  __shared__ uint32_t ws[4][2];
  const Pick P = pick_and_scan(rx_len, mask, n_streams, min_len, ws);
  if (threadIdx.x == 0u) pairs[blockIdx.x] = make_uint2(P.tot_s, P.tot_b);
}

// pairs[0 .. n_pairs): {streams, bytes} of each workgroup -> the same, summed over the workgroups before it
__global__ __launch_bounds__(256) void drain_scan_kernel(uint2 *__restrict__ pairs, uint32_t n_pairs, uint32_t cap_streams, uint64_t cap_bytes,
                                                         uint32_t *__restrict__ totals) {
  __shared__ uint32_t ws[4][2];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t carry_s = 0u, carry_b = 0u;
  for (uint32_t base = 0; base < n_pairs; base += 256u) {   // (the same trip count in every lane: barriers below)
    const uint32_t i = base + threadIdx.x;
    const uint2 v = i < n_pairs ? pairs[i] : make_uint2(0u, 0u);
    const uint32_t is = wave_scan(v.x, lane), ib = wave_scan(v.y, lane);
    if (lane == 63u) { ws[wv][0] = is; ws[wv][1] = ib; }
    __syncthreads();
    uint32_t ps = carry_s + is - v.x, pb = carry_b + ib - v.y;
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) {
      const uint32_t cs = ws[w][0], cb = ws[w][1];
      if (w < wv) { ps += cs; pb += cb; }
      carry_s += cs; carry_b += cb;
    }
    if (i < n_pairs) pairs[i] = make_uint2(ps, pb);
    __syncthreads();
  }
  if (threadIdx.x == 0u) {
    totals[0] = carry_s;
    totals[1] = carry_b;
    totals[2] = carry_s <= cap_streams && (uint64_t)carry_b <= cap_bytes ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void drain_pack_kernel(ProcState T, const uint8_t *__restrict__ mask, uint32_t n_streams, uint32_t min_len,
                                                         const uint2 *__restrict__ pairs, const uint32_t *__restrict__ totals,
                                                         uint32_t *__restrict__ streams, uint32_t *__restrict__ offsets, uint8_t *__restrict__ data) {
  __shared__ uint32_t ws[4][2];
  __shared__ SpanJob jobs[4][64];
  if (totals[2] == 0u) return;   // a cap is too small: nothing is drained (the same word for every lane of the grid)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cap = T.rx_cap;
  const Pick P = pick_and_scan(T.rx_len, mask, n_streams, min_len, ws);
  const uint2 base = pairs[blockIdx.x];
  if (blockIdx.x == 0u && threadIdx.x == 0u && offsets) offsets[totals[0]] = totals[1];
  uint32_t r = 0u;
  const uint32_t dst = base.y + P.pos_b;
  if (P.sel) {
    r = T.rx_r[s];
    streams[base.x + P.pos_s] = s;
    offsets[base.x + P.pos_s] = dst;
  }
  // the wave's selected rings, compacted
  const uint64_t vote = __builtin_amdgcn_ballot_w64(P.sel);
  const uint32_t n_jobs = (uint32_t)__builtin_popcountll(vote);
  if (P.sel) jobs[wv][__builtin_popcountll(vote & ((1ull << lane) - 1ull))] = SpanJob{s, r, P.len, dst};
  uint32_t longest = P.sel ? P.len : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, o, 64));
  __syncthreads();
  const uint32_t lps = lanes_per_span(longest), spp = 64u / lps;   // lanes per span, spans per pass
  const uint32_t sub = lane / lps, k0 = lane % lps;
  for (uint32_t p = 0; p < n_jobs; p += spp * kInFlight) {
    SpanJob J[kInFlight];
    uint32_t most = 0u;
#pragma unroll
    for (uint32_t u = 0; u < kInFlight; u++) {
      const uint32_t slot = p + u * spp + sub;
      J[u] = slot < n_jobs ? jobs[wv][slot] : SpanJob{0u, 0u, 0u, 0u};
      most = max(most, J[u].len);
    }
    for (uint32_t k = k0; k < most; k += lps) {
      uint8_t v[kInFlight];
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++) {
        if (k < J[u].len) {
          const uint32_t room = cap - J[u].start;   // bytes up to the ring's end; the span continues at the ring's start
          v[u] = T.rx_buf[(size_t)J[u].src * cap + (k < room ? J[u].start + k : k - room)];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++)
        if (k < J[u].len) data[(size_t)J[u].dst + k] = v[u];
    }
  }
  if (P.sel) {   // readIndex advanced by _length modulo the capacity (a full ring comes back to where it was), _length = 0
    const uint32_t room = cap - r;
    T.rx_r[s] = P.len < room ? r + P.len : P.len - room;
    T.rx_len[s] = 0u;
  }
}

uint32_t groups_of(uint32_t n_streams) { return n_streams ? (n_streams + 255u) / 256u : 1u; }   // (an empty batch still writes its totals)

}  // namespace

hipError_t launch_drain_totals(uint32_t *d_pairs, uint32_t n_pairs, uint32_t cap_streams, uint64_t cap_bytes, uint32_t *d_totals, hipStream_t st) {
  hipLaunchKernelGGL(drain_scan_kernel, dim3(1), dim3(256), 0, st, (uint2 *)d_pairs, n_pairs, cap_streams, cap_bytes, d_totals);
  return hipGetLastError();
}

size_t drain_sparse_pair_words(uint32_t n_streams) { return 2u * (size_t)groups_of(n_streams); }

hipError_t launch_drain_sparse_size(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, uint32_t min_len, uint32_t cap_streams, uint64_t cap_bytes,
                                    uint32_t *d_pairs, uint32_t *d_totals, hipStream_t st) {
  const uint32_t groups = groups_of(n_streams);
  hipLaunchKernelGGL(drain_count_kernel, dim3(groups), dim3(256), 0, st, T.rx_len, d_mask, n_streams, min_len, (uint2 *)d_pairs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_drain_totals(d_pairs, groups, cap_streams, cap_bytes, d_totals, st);
}

hipError_t launch_drain_sparse_pack(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, uint32_t min_len, const uint32_t *d_pairs,
                                    const uint32_t *d_totals, uint32_t *d_streams, uint32_t *d_offsets, uint8_t *d_data, hipStream_t st) {
  hipLaunchKernelGGL(drain_pack_kernel, dim3(groups_of(n_streams)), dim3(256), 0, st, T, d_mask, n_streams, min_len, (const uint2 *)d_pairs, d_totals, d_streams,
                     d_offsets, d_data);
  return hipGetLastError();
}

}  // namespace fsk
