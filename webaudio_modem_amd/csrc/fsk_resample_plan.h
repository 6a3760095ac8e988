// fsk_resample_plan.h -- the host arithmetic of the resampler (fsk_resample.hip, include/fskhip_next.h: fskhip_resampler_*), in
// plain C++ so that it also compiles without HIP (tests/cpp/resample_plan_check.cpp): the history a handle keeps, what a call
// writes, and how a launch cuts its work into workgroups and sizes their LDS.  Not part of the ABI.
//
// Up (factor L, n_taps taps):   out[t] = sum c[i] x[(t - i) / L] over the i with (t - i) a multiple of L.  Output t = mL + p only
//   meets the taps of phase p, c[p + kL] with input x[m - k]; phase p has resample_phase_taps(L, n_taps, p) of them and the
//   longest has K = ceil(n_taps / L).  The handle keeps the taps phase by phase, [L][K], and the last
//   H = ceil((n_taps - 1) / L) >= K - 1 inputs of every stream.
// Down:                         y[k] = sum c[i] u[kL - i].  The handle keeps the last n_taps - 1 inputs.  A workgroup stages them by
//   residue: input tt (counted from kL0 - Hp, Hp = n_taps - 1 rounded up to a multiple of L) lies at [tt % L][tt / L] of an
//   [L][Q] array, so that the 64 outputs of a wave read 64 consecutive words for every tap.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fsk {

constexpr uint32_t kResampleThreads = 256;        // four waves per workgroup
constexpr uint32_t kResampleMaxFactor = 32;
constexpr uint32_t kResampleMaxTaps = 4096;
constexpr uint32_t kResampleLdsBytes = 65536;     // what a workgroup may take without asking for more
constexpr uint32_t kResampleUpSeg = 1024;         // inputs of one stream per workgroup, stream-major
constexpr uint32_t kResampleTile = 64;            // inputs (up) / outputs (down) per stream per workgroup, sample-major
constexpr uint32_t kResampleDownSpan = 8192;      // inputs of one stream per workgroup at most, stream-major (down)

// floats of history per stream: direction 0 = up, 1 = down
inline uint32_t resample_history(int direction, uint32_t L, uint32_t n_taps) {
  return direction == 0 ? (n_taps - 1 + L - 1) / L : n_taps - 1;
}
// elements per stream a call writes for n_in per stream (down: n_in is a multiple of L)
inline size_t resample_out_count(int direction, uint32_t L, size_t n_in) { return direction == 0 ? n_in * L : n_in / L; }
inline uint32_t resample_phase_len(uint32_t L, uint32_t n_taps) { return (n_taps + L - 1) / L; }          // K
inline uint32_t resample_phase_taps(uint32_t L, uint32_t n_taps, uint32_t p) { return p < n_taps ? (n_taps - p + L - 1) / L : 0u; }
// low-rate samples of a modulated signal of `len` samples behind a decimator: the signal and the filter's ringing
inline size_t resample_down_length(uint32_t L, uint32_t n_taps, size_t len) { return (len + n_taps - 1 + L - 1) / L; }

// One launch.  A workgroup takes ns = 1 << log2_ns streams x seg inputs (up) or outputs (down) of each.  split: workgroups per
// row (stream-major) / stream tiles per segment (sample-major); the grid is one-dimensional, blocks = 0 where it is more than one
// launch takes.  x_pitch: floats of LDS per staged stream.  Up: x_pitch >= hist + seg; behind the ns rows come the four waves'
// output rows of 64 L floats.  Down: x_pitch = L * q_len, hist_pad = Hp; behind the rows comes the [64][ns + 1] tile the
// sample-major layout leaves through.
struct ResamplePlan {
  uint32_t hist, hist_pad, seg, log2_ns, x_pitch, q_len, split;
  uint64_t blocks;
  size_t lds_bytes;
};

// the grid of a plan (this one or fsk_ratecvt_plan.h's) whose workgroups take `seg` of a stream's n_units each
template <class Plan>
inline void resample_grid(Plan &P, uint32_t seg, bool stream_major, uint32_t n_streams, size_t n_units) {
  const uint64_t segs = (n_units + seg - 1) / seg, ns = 1u << P.log2_ns;
  const uint64_t tiles = (n_streams + ns - 1) / ns;
  P.split = (uint32_t)(stream_major ? segs : tiles);
  P.blocks = stream_major ? segs * n_streams : segs * tiles;
  if (P.blocks > 0x7FFFFFFFull || segs > 0x7FFFFFFFull) P.blocks = 0;
}

// n_in: inputs per stream (> 0)
inline ResamplePlan resample_up_plan(bool stream_major, uint32_t L, uint32_t n_taps, uint32_t n_streams, size_t n_in) {
  ResamplePlan P{};
  P.hist = P.hist_pad = resample_history(0, L, n_taps);
  P.seg = stream_major ? kResampleUpSeg : kResampleTile;
  P.x_pitch = (P.hist + P.seg) | 1u;   // odd: the streams of a sample-major tile start on different banks
  const size_t out_floats = (size_t)(kResampleThreads / 64u) * 64u * L;
  P.log2_ns = 0;
  if (!stream_major)
    while (P.log2_ns < 6 && sizeof(float) * (((size_t)2u << P.log2_ns) * P.x_pitch + out_floats) <= kResampleLdsBytes) P.log2_ns++;
  P.lds_bytes = sizeof(float) * (((size_t)1u << P.log2_ns) * P.x_pitch + out_floats);
  resample_grid(P, P.seg, stream_major, n_streams, n_in);
  return P;
}

// n_out: outputs per stream (> 0)
inline ResamplePlan resample_down_plan(bool stream_major, uint32_t L, uint32_t n_taps, uint32_t n_streams, size_t n_out) {
  ResamplePlan P{};
  P.hist = resample_history(1, L, n_taps);
  P.hist_pad = (P.hist + L - 1) / L * L;
  uint32_t seg = kResampleDownSpan / L / 64u * 64u;
  seg = seg > 1024u ? 1024u : seg;
  P.seg = stream_major ? seg : kResampleTile;
  P.q_len = P.hist_pad / L + P.seg;
  P.x_pitch = L * P.q_len;
  P.log2_ns = 0;
  if (!stream_major)
    while (P.log2_ns < 6 && sizeof(float) * (((size_t)2u << P.log2_ns) * P.x_pitch + 64u * ((2u << P.log2_ns) + 1u)) <= kResampleLdsBytes) P.log2_ns++;
  P.lds_bytes = sizeof(float) * (((size_t)1u << P.log2_ns) * P.x_pitch + (stream_major ? 0u : 64u * ((1u << P.log2_ns) + 1u)));
  resample_grid(P, P.seg, stream_major, n_streams, n_out);
  return P;
}

}  // namespace fsk
