// fsk_processor_rate_plan.h -- how fskhip_processor_process_rate_* (fsk_processor_rate.hip) and, at the end of the file,
// fskhip_processor_process_ratecvt_* (fsk_processor_ratecvt.hip) run their TX sides, in plain C++ so that it also compiles without
// HIP (tests/cpp/processor_rate_plan_check.cpp, processor_ratecvt_plan_check.cpp).  Not part of the ABI.
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

}  // namespace fsk
