// fsk_pick_dev.h -- the in-workgroup half of a compaction, shared by the kernels that list some of a batch's streams and pack a
// run of bytes per listed stream (fsk_drain.hip: the compacted RX drain; fsk_xmodem_rx.hip: the resident XModem receiver):
// every lane brings whether its stream is picked and how many bytes it contributes, and learns its place among the workgroup's
// picked streams and bytes.  256 lanes per workgroup, no atomics: ballot + popcount, a wave prefix sum, LDS across the four waves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsk {

// inclusive prefix sum over the wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)x, o, 64);
    if (lane >= o) x += t;
  }
  return x;
}

// What a lane learns about its stream s = blockIdx.x * 256 + threadIdx.x: whether it is selected, and where the workgroup's
// selected streams / bytes before it end (pos_s, pos_b) out of the workgroup's totals (tot_s, tot_b).
struct Pick {
  bool sel;
  uint32_t len, pos_s, pos_b, tot_s, tot_b;
};
// sel: the lane's stream is picked; len: its byte count (counted only where sel).  Every lane of the workgroup calls it (a barrier).
__device__ __forceinline__ Pick pick_scan(bool sel, uint32_t len, uint32_t (*ws)[2]) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  Pick P;
  P.len = len;
  P.sel = sel;
  const uint32_t b = P.sel ? P.len : 0u;
  const uint64_t vote = __builtin_amdgcn_ballot_w64(P.sel);
  const uint32_t incl = wave_scan(b, lane);
  if (lane == 63u) { ws[wv][0] = (uint32_t)__builtin_popcountll(vote); ws[wv][1] = incl; }
  __syncthreads();
  P.pos_s = (uint32_t)__builtin_popcountll(vote & ((1ull << lane) - 1ull));
  P.pos_b = incl - b;
  P.tot_s = 0u; P.tot_b = 0u;
#pragma unroll
  for (uint32_t w = 0; w < 4u; w++) {
    const uint32_t cs = ws[w][0], cb = ws[w][1];
    if (w < wv) { P.pos_s += cs; P.pos_b += cb; }
    P.tot_s += cs; P.tot_b += cb;
  }
  return P;
}

// lanes a wave puts on one span when its longest span has `longest` bytes: the next power of two, at most 64
__device__ __forceinline__ uint32_t lanes_per_span(uint32_t longest) {
  uint32_t l = 1u;
  while (l < longest && l < 64u) l <<= 1;
  return l;
}

struct SpanJob { uint32_t src, start, len, dst; };   // bytes [start, start + len) modulo the capacity of ring src -> data[dst ..]

}  // namespace fsk
