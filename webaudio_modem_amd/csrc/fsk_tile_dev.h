// fsk_tile_dev.h -- wave code that demod_pipe_kernel (fsk_pipe.hip) and the four-wave kernels (fsk_blk.hip) share around the
// per-sample arithmetic of fsk_pipe_dev.h: the asm tile prefetch with its hand-counted waits and the front wave's state
// stores; and the amplitude ring's descriptor, which every fp32 whole-tile kernel builds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fsk_params.h"
#include "fsk_dev.h"
#include "fsk_pipe_dev.h"

namespace fsk {

// ---- the tile prefetch: three tiles in flight, in three register sets used in turn ----------------------------------
// A group's sample rows are one buffer (in_rsrc: [rows in the batch][pitch] floats).  Lane (sub_row, chunk) = (lane / 4,
// lane % 4) loads 16 bytes -- samples 4 chunk .. 4 chunk + 3 -- of rows sub_row, + 16, + 32, + 48: in_voff is its byte offset
// within the first sixteen rows, in_row16 the bytes from a row to the row sixteen below.  Rows beyond the buffer read as
// 0: the row step rides in the bounds-checked VGPR offset.
// The loads are inline asm with hand-counted waits: vmcnt counts in issue order and hipcc, which cannot see across a
// loop's back edge, would drain everything (vmcnt(0)) at the top of every iteration.  They land asynchronously: between
// issue and the covering wait nothing may touch the destination registers, so the sets are passed by reference and the
// callers' loops are unrolled by three so that no set is ever copied (tools/check_isa.py proves it on the compiled kernels).
__device__ __forceinline__ void tile_load1(const v4i &in_rsrc, uint32_t in_voff, uint32_t in_row16, uint32_t rows16, uint32_t soff, v4f &dst) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(in_voff + rows16 * in_row16), "s"(in_rsrc), "s"(soff) : "memory");
}
// tile t of this launch's (or time slice's) n_tiles, which begin at tile t_begin of the call; beyond the last one the
// last is loaded again, so that every tile issues its prefetch and the counts stay fixed
__device__ __forceinline__ void tile_load(const v4i &in_rsrc, uint32_t in_voff, uint32_t in_row16, size_t t, size_t n_tiles, uint32_t t_begin,
                                          v4f &a, v4f &b, v4f &c, v4f &d) {
  const uint32_t tn = (uint32_t)((t_begin + (t < n_tiles ? t : n_tiles - 1)) * kFastTile * 4u);
  tile_load1(in_rsrc, in_voff, in_row16, 0u, tn, a); tile_load1(in_rsrc, in_voff, in_row16, 1u, tn, b);
  tile_load1(in_rsrc, in_voff, in_row16, 2u, tn, c); tile_load1(in_rsrc, in_voff, in_row16, 3u, tn, d);
}
// Everything issued so far has landed.  Before the tile loop: the loop may receive the sets in other registers than the
// loads were issued into, and any such copy must see landed data.  After it: the last prefetches are still in flight and
// their registers are dead to the compiler -- keep them until they land.
__device__ __forceinline__ void tile_fence(v4f &a0, v4f &a1, v4f &a2, v4f &a3, v4f &b0, v4f &b1, v4f &b2, v4f &b3,
                                           v4f &c0, v4f &c1, v4f &c2, v4f &c3) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3),
               "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3) : : "memory");
}
// A set goes to its place in the staging tile [4 chunks][kSlotStride] v4f (st_slot = chunk * kSlotStride + sub_row) while the
// two sets issued after it (8 loads) may still be in flight, plus, in the write-back variant, this wave's stores of the two
// tiles in between (4 each).
template <bool WB>
__device__ __forceinline__ void tile_stage(v4f *stage, uint32_t st_slot, v4f &r0, v4f &r1, v4f &r2, v4f &r3) {
  if (WB) asm volatile("s_waitcnt vmcnt(16)" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3) : : "memory");
  else asm volatile("s_waitcnt vmcnt(8)" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3) : : "memory");
  stage[st_slot] = r0; stage[st_slot + 16] = r1; stage[st_slot + 32] = r2; stage[st_slot + 48] = r3;
}

// ---- the front wave's epilogue: AGC gain and pre-filter history (the I/Q low-pass state goes through pipe_store) ----------
template <int COH>
__device__ __forceinline__ void front_store(const FrontLane &F, const PipeCtx &C) {
  const __amdgpu_buffer_rsrc_t rs_rsrc = C.rs_rsrc;
  const FastMem &M = C.M;
  const uint32_t fld = C.fld;
  PIPE_RSTORE(agc_gain, F.g);
  PIPE_RSTORE(bp_x1, F.bx1); PIPE_RSTORE(bp_x2, F.bx2); PIPE_RSTORE(bp_y1, F.by1); PIPE_RSTORE(bp_y2, F.by2);
}

// ---- the amplitude ring as the back / frame wave writes it (layout: fsk_dev.h); wrap = bytes of the ring ------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t amp_ring_rsrc(const DemodState &S, uint32_t wrap) {
  return __builtin_amdgcn_make_buffer_rsrc(S.amp_ring, 0, (int)wrap, 0x00020000);
}

}  // namespace fsk
