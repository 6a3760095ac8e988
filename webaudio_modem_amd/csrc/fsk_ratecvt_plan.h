// fsk_ratecvt_plan.h -- the host arithmetic of the rational rate converter (fsk_ratecvt.hip, include/fskhip_next.h:
// fskhip_ratecvt_*), in plain C++ so that it also compiles without HIP (tests/cpp/ratecvt_plan_check.cpp): the history a handle
// keeps, what a call writes, the per-period table, and how a launch cuts its work into workgroups and sizes their LDS.  Not part
// of the ABI.
//
// Up factor L, down factor M (coprime), n_taps taps:  y[j] = sum_k c[p + kL] x[m - k],  p = (jM) mod L,  m = (jM) div L.  L outputs
// and M inputs make a period: output q of a period has phase (qM) mod L -- every phase once, L and M being coprime -- and its
// newest input lies (qM) div L behind the period's first.  Phase p has resample_phase_taps() taps, the longest K = ceil(n_taps / L)
// (resample_phase_len), and the handle keeps the last H = ceil((n_taps - 1) / L) >= K - 1 inputs of every stream: the
// interpolator's, resample_history(0, L, n_taps) (fsk_resample_plan.h).  The taps lie in OUTPUT order on the
// device, [K][L] with column q holding phase (qM) mod L, so that the consecutive outputs of a wave read consecutive words.
//
// A workgroup takes whole periods.  It computes `rows` rows of G periods each, four rows to a lane (the same place q in four
// periods: one tap read, four products), from inputs staged in LDS behind H floats of history:
//   stream-major   one stream, rows = 4 consecutive blocks of G periods; LDS holds H + 4 G M floats
//   sample-major   ns = 1 << log2_ns streams of one block each; LDS holds ns rows of x_pitch >= H + G M floats (x_pitch odd, so
//                  that the streams of a frame land on different banks), and PLAYBACK a [G L][ns + 1] tile behind them through
//                  which the frames leave
//
// Calls of any length.  A handle carries a position pos in [0, M): the inputs taken since the last period boundary, one word for
// all its streams, 0 at creation and after a reset of all streams.  A call of n inputs is laid on the period grid as if it began
// pos inputs before its first sample: input t of the call is input pos + t of the grid, the grid's outputs are numbered from the
// boundary, and the call owns those whose newest input (jM) div L lies in [pos, pos + n): j from q0 = ceil(pos L / M) up to
// ceil((pos + n) L / M), written at column j - q0.  Where L < M that can be none; the call still advances position and history.
// The launch covers ceil((pos + n) / M) periods with the same workgroups, staged from H + pos inputs in front of the call: the first
// workgroup's pos words in front of the history hold nothing, and the places outside the call's outputs are skipped, so none of them is
// read (an owned output reads no further back than pos - H of the grid).  Afterwards pos is (pos + n) mod M.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fsk_resample_plan.h"

namespace fsk {

constexpr uint32_t kRatecvtMaxFactor = 256;       // L and M
constexpr uint32_t kRatecvtRowOutputs = 1024;     // outputs per row of a stream-major workgroup, about
constexpr uint32_t kRatecvtTileOutputs = 64;      // outputs per stream of a sample-major workgroup, about

inline uint32_t ratecvt_gcd(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }
// elements per stream a call writes for n_in per stream (a multiple of M)
inline size_t ratecvt_out_count(uint32_t L, uint32_t M, size_t n_in) { return n_in / M * L; }
// the first output of the period grid that a call from position pos owns: ceil(pos L / M)
inline size_t ratecvt_first_output(uint32_t L, uint32_t M, size_t pos) { return (pos * L + M - 1) / M; }
// elements per stream a call of n_in per stream writes from position pos (any n_in; pos = 0 and n_in = kM: kL)
inline size_t ratecvt_out_count_any(uint32_t L, uint32_t M, uint32_t pos, size_t n_in) {
  return ratecvt_first_output(L, M, (size_t)pos + n_in) - ratecvt_first_output(L, M, pos);
}
// the smallest n_in with ratecvt_out_count_any(pos, n_in) >= n_out: the newest input of the last output wanted, and itself
inline size_t ratecvt_in_count_any(uint32_t L, uint32_t M, uint32_t pos, size_t n_out) {
  return n_out ? (ratecvt_first_output(L, M, pos) + n_out - 1) * M / L + 1 - pos : 0;
}
inline uint32_t ratecvt_next_position(uint32_t M, uint32_t pos, size_t n_in) { return (uint32_t)(((size_t)pos + n_in) % M); }
// outputs that can be non-zero for a signal of `len` inputs: the last input meets the last tap at stuffed index (len - 1) L + n_taps - 1
inline size_t ratecvt_out_length(uint32_t L, uint32_t M, uint32_t n_taps, size_t len) { return len ? ((len - 1) * L + n_taps - 1) / M + 1 : 0; }
// output q of a period: its phase and how far its newest input lies behind the period's first
inline uint32_t ratecvt_phase(uint32_t L, uint32_t M, uint32_t q) { return q * M % L; }
inline uint32_t ratecvt_offset(uint32_t L, uint32_t M, uint32_t q) { return q * M / L; }
// the table the kernels read, one word per q: offset | phase << 16
inline uint32_t ratecvt_table_word(uint32_t L, uint32_t M, uint32_t q) { return ratecvt_offset(L, M, q) | ratecvt_phase(L, M, q) << 16; }

// One launch.  seg_periods = periods per workgroup (rows x G stream-major, G sample-major); row_stride: floats of LDS between
// two rows (G M stream-major, x_pitch sample-major); span: floats staged per stream (H + seg_periods M).  split: workgroups per
// stream (stream-major) / stream tiles per segment (sample-major); the grid is one-dimensional, blocks = 0 where it is more
// than one launch takes.  tile_words: the words of the sample-major PLAYBACK tile (0 otherwise).
struct RatecvtPlan {
  uint32_t hist, G, rows, log2_ns, x_pitch, row_stride, span, seg_periods, split, tile_words;
  uint64_t blocks;
  size_t lds_bytes;
};

inline size_t ratecvt_tile_lds(uint32_t H, uint32_t L, uint32_t M, uint32_t G, uint32_t log2_ns, bool tile) {
  const size_t ns = (size_t)1u << log2_ns, x_pitch = (H + G * M) | 1u;
  return sizeof(float) * (ns * x_pitch + (tile ? (size_t)G * L * (ns + 1u) : 0u));
}

// a workgroup's shape, all of a plan but its grid; playback: the direction that leaves in the format (it alone needs the tile)
inline RatecvtPlan ratecvt_shape(bool stream_major, bool playback, uint32_t L, uint32_t M, uint32_t n_taps) {
  RatecvtPlan P{};
  const uint32_t H = P.hist = resample_history(0, L, n_taps);
  if (stream_major) {
    P.rows = 4;
    P.G = kRatecvtRowOutputs / L ? kRatecvtRowOutputs / L : 1u;
    while (P.G > 1 && sizeof(float) * ((size_t)H + 4u * P.G * M) > kResampleLdsBytes * 3u / 4u) P.G--;
    P.log2_ns = 0;
    P.seg_periods = 4u * P.G;
    P.span = H + P.seg_periods * M;
    P.x_pitch = P.span;
    P.row_stride = P.G * M;
    P.tile_words = 0;
    P.lds_bytes = sizeof(float) * (size_t)P.span;
  } else {
    // as many streams as fit, up to 64; a block is halved while fewer than 16 streams fit beside it
    P.G = kRatecvtTileOutputs / L ? kRatecvtTileOutputs / L : 1u;
    for (;;) {
      P.log2_ns = 0;
      while (P.log2_ns < 6 && ratecvt_tile_lds(H, L, M, P.G, P.log2_ns + 1u, playback) <= kResampleLdsBytes) P.log2_ns++;
      if (P.G == 1 || (P.log2_ns >= 4 && ratecvt_tile_lds(H, L, M, P.G, P.log2_ns, playback) <= kResampleLdsBytes)) break;
      P.G = (P.G + 1u) / 2u;
    }
    P.rows = 1u << P.log2_ns;
    P.seg_periods = P.G;
    P.span = H + P.G * M;
    P.x_pitch = P.span | 1u;
    P.row_stride = P.x_pitch;
    P.tile_words = playback ? P.G * L * (P.rows + 1u) : 0u;
    P.lds_bytes = ratecvt_tile_lds(H, L, M, P.G, P.log2_ns, playback);
  }
  return P;
}

// n_in: inputs per stream (> 0, any), from position pos < M: the periods that hold inputs [pos, pos + n_in) of the grid, n_in / M
// of them for whole periods from a boundary
inline RatecvtPlan ratecvt_plan(bool stream_major, bool playback, uint32_t L, uint32_t M, uint32_t n_taps, uint32_t n_streams, uint32_t pos, size_t n_in) {
  RatecvtPlan P = ratecvt_shape(stream_major, playback, L, M, n_taps);
  resample_grid(P, P.seg_periods, stream_major, n_streams, ((size_t)pos + n_in + M - 1) / M);
  return P;
}

}  // namespace fsk
