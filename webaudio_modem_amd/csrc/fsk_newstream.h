// fsk_newstream.h -- the state words of a NEW stream that joins a live engine: new FSKCore() + configure() (fsk.ts:101-131,
// 175-188) as fsk_create.hip's init_kernel writes it, placed on the engine's ring grid and, on fp32 engines of one shared
// configuration, in the engine's free-running I/Q frame.  The one definition behind map[i] = -1 of fskhip_remap_streams
// (fsk_remap.hip) and of fskhip_restore_streams (fsk_snapshot.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fsk_params.h"

namespace fsk {

// Where a new stream starts.  grid: its ring positions are the engine's (an engine in lock step has ONE position for every
// stream; a ring of length 0 reads nothing before its own pushes).  frame: fp32 engines of one shared configuration keep the
// I/Q low-pass in ONE free-running frame (fsk_pipe_dev.h pipe_free0: NCO phase minus frame offset, wave-uniform) of phase
// fr0 (64-bit turns): a new stream joins it as fskhip_reset places a stream there -- its NCO at 0, its frame offset minus the
// frame's phase, lastPhase = 0 expressed in the frame (fsk_api.hip reset_kernel).
struct NewStream {
  uint32_t matched_zero;          // `matched` for an all-zero bit history (what configure() leaves)
  uint32_t grid, poly_phase, amp_pos;
  uint32_t frame;
  uint64_t fr0;
};

template <typename Real>
__device__ __forceinline__ Real new_stream_real(int f, const NewStream &N) {
  if (f == RF_last_phase && N.frame) {
    double ph = (double)N.fr0 * 5.42101086242752217e-20 * 6.283185307179586476925;
    ph = ph > 3.14159265358979323846 ? ph - 6.283185307179586476925 : ph;
    return (Real)ph;
  }
  return (f == RF_agc_gain || f == RF_nco_c) ? (Real)1.0 : f == RF_sil_thr ? (Real)0.01 : (Real)0;
}

__device__ __forceinline__ uint32_t new_stream_int(int f, const NewStream &N) {
  if (N.grid && f == IF_poly_phase) return N.poly_phase;
  if (N.grid && f == IF_amp_pos) return N.amp_pos;
  if (N.frame && (f == IF_fr_lo || f == IF_fr_hi)) {
    const uint64_t noff = 0ull - N.fr0;
    return f == IF_fr_lo ? (uint32_t)noff : (uint32_t)(noff >> 32);
  }
  return f == IF_matched ? N.matched_zero : f == IF_bit_wait ? kBigWait : f == IF_zr_dph ? kHandPairs : 0u;
}

// the frame's phase as a stream's state words hold it: NCO phase minus frame offset
__host__ __device__ inline uint64_t frame_phase(uint32_t nco_lo, uint32_t nco_hi, uint32_t fr_lo, uint32_t fr_hi) {
  return (((uint64_t)nco_hi << 32) | nco_lo) - (((uint64_t)fr_hi << 32) | fr_lo);
}

}  // namespace fsk
