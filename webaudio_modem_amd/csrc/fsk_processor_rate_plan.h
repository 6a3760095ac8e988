// fsk_processor_rate_plan.h -- how fskhip_processor_process_rate_* (fsk_processor_rate.hip) and, at the end of the file,
// fskhip_processor_process_ratecvt_* (fsk_processor_ratecvt.hip) run their TX sides, in plain C++ so that it also compiles without
// HIP (tests/cpp/processor_rate_plan_check.cpp, processor_ratecvt_plan_check.cpp, processor_ratecvt_any_plan_check.cpp).  Not part
// of the ABI.
//
// The fused kernel (fsk_mod.hip: processor_io_rate_kernel) is one wave per 64 streams, lane = stream.  The generator's samples go
// into a delay line in LDS, [slot][lane] with rows kRateLanePitch words apart, which at entry holds the decimator's history
// (n_taps - 1 samples per stream) and behind it takes the quantum's samples kRateChunk at a time -- the generator's step -- so it
// needs n_taps - 1 + max(Ld, kRateChunk) slots: the history an output reaches back to and what is generated before the output is
// taken; behind it lie the packed code rows of 32 outputs per stream.  The two launches the kernel replaces -- processor_io_kernel
// into a float tile, then resample_down_kernel -- are taken by a filter whose delay line does not fit the budget, and by
// interleaved frames (sample-major): at 262 144 streams, factor 6 and 97 taps the pair measured 3.9 / 4.2 ms for quanta of 80 / 160
// stream-major, where the fused kernel takes 1.6 / 2.9 ms, but 1.2 / 2.0 ms sample-major, where a fused kernel storing frames from
// its registers took 1.35 / 2.5 ms (profiles/processor_rate_bench.jsonl).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fsk_ratecvt_plan.h"

namespace fsk {

constexpr uint32_t kRateLdsBytes = 65536;    // what a workgroup may take without asking for more
constexpr uint32_t kRateLanePitch = 65;      // odd: the history's transposed load and store meet every bank once per half wave
constexpr uint32_t kRateChunk = 4;           // samples per step of the generator (frame_next4)
constexpr uint32_t kRateCodeTile = 32;       // outputs per stream per flush of the code rows (stream-major)

struct RatePlan {
  bool fits;           // the delay line and the code rows are within the budget
  bool fused;          // one launch: it fits and the layout is stream-major
  uint32_t slots;      // samples per stream the delay line holds
  uint32_t code_words; // words of packed code rows behind it
  size_t lds_bytes;    // of the fused kernel, whether or not it fits
};

// words between the code rows of two streams: the tile's words and one, odd
inline uint32_t rate_code_pitch(uint32_t esz) { return kRateCodeTile * esz / 4u + 1u; }

// Ld: the decimator's factor; esz: bytes per output element (1, 2 or 4)
inline RatePlan processor_rate_plan(uint32_t Ld, uint32_t n_taps, uint32_t esz, bool stream_major) {
  RatePlan P{};
  P.slots = n_taps - 1u + (Ld > kRateChunk ? Ld : kRateChunk);
  P.code_words = 64u * rate_code_pitch(esz);
  P.lds_bytes = sizeof(uint32_t) * ((size_t)P.slots * kRateLanePitch + P.code_words);
  P.fits = P.lds_bytes <= kRateLdsBytes;
  P.fused = P.fits && stream_major;
  return P;
}

// The same for fskhip_processor_process_ratecvt_* (fsk_processor_ratecvt.hip) and its fused kernel (fsk_mod.hip:
// processor_io_ratecvt_kernel), whose filter is a playback converter's (fsk_ratecvt_plan.h): up factor L, n_taps taps.  Output j's
// newest input is m = (jM) div L and its sum reaches back K - 1 <= H = ceil((n_taps - 1) / L) inputs from there, so the delay line
// holds the handle's history of H samples per stream and behind it the generator's step: H + kRateChunk slots, whatever M is --
// an output is taken as soon as sample m is written, and no sample is written over before the outputs that end at most
// kRateChunk - 1 samples before it have read their H samples back.  The pair is processor_io_kernel into a float tile, then
// ratecvt_playback_kernel.
inline RatePlan processor_ratecvt_plan(uint32_t L, uint32_t n_taps, uint32_t esz, bool stream_major) {
  RatePlan P{};
  P.slots = (n_taps - 1u + L - 1u) / L + kRateChunk;
  P.code_words = 64u * rate_code_pitch(esz);
  P.lds_bytes = sizeof(uint32_t) * ((size_t)P.slots * kRateLanePitch + P.code_words);
  P.fits = P.lds_bytes <= kRateLdsBytes;
  P.fused = P.fits && stream_major;
  return P;
}

// Where the fused kernel's ANY form starts: a quantum of n_out outputs from the playback handle's position pos < M, the engine
// samples taken since the last period boundary (fsk_ratecvt_plan.h: "Calls of any length").  The kernel takes the grid's outputs in
// order, each as soon as its newest input is written, so it needs the first one the call owns and that output's accumulators:
//   k0      ceil(pos L / M), the first output of the period grid whose newest input lies in the call (at most L)
//   q       k0 mod L, its column of the [K][L] tap table
//   ph      (k0 M) mod L, its phase
//   m       (k0 M) div L - pos, its newest input counted from the call's first sample (>= 0 by the choice of k0)
//   n_high  ratecvt_in_count_any(L, M, pos, n_out): the engine samples the call generates, the newest input of output
//           k0 + n_out - 1 and itself
// The whole-period form is pos = 0 with n_out a multiple of L over n_out / L * M samples: k0, q, ph and m are zero.
struct RatecvtStart {
  size_t k0;
  uint32_t q, ph, m;
  size_t n_high;
};
inline RatecvtStart processor_ratecvt_start(uint32_t L, uint32_t M, uint32_t pos, size_t n_out) {
  RatecvtStart s{};
  s.k0 = ratecvt_first_output(L, M, pos);
  s.q = (uint32_t)(s.k0 % L);
  s.ph = (uint32_t)(s.k0 * M % L);
  s.m = (uint32_t)(s.k0 * M / L - pos);
  s.n_high = ratecvt_in_count_any(L, M, pos, n_out);
  return s;
}
// which of the two forms a quantum of n_high engine samples runs: whole periods from a period boundary keep their own
// instantiations.  (Where L < M the fewest samples that write whole periods of output stop short of the last period's end --
// 159 of 160 for one period of 147 / 160 -- so the any-length call of such an n_out is the ANY form's.)
inline bool processor_ratecvt_any(uint32_t L, uint32_t M, uint32_t pos, size_t n_out, size_t n_high) {
  return pos != 0 || n_out % L != 0 || n_high != n_out / L * M;
}

}  // namespace fsk
