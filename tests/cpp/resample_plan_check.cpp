// resample_plan_check.cpp -- the resampler's host arithmetic (webaudio_modem_amd/csrc/fsk_resample_plan.h) from a program of its
// own, for a sanitizer run without a GPU: every factor 1..32 x every tap count 1..4096 x both layouts x both directions.
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I webaudio_modem_amd/csrc
//     tests/cpp/resample_plan_check.cpp -o resample_plan_check && ./resample_plan_check
// Checked: the histories hold what a filter of that length reaches back to; the phases' tap counts add up; a workgroup's LDS fits
// and holds every index the kernels form; the workgroups of a launch cover every sample once; and, by walking them, that every
// entry of the next history is written by exactly one staged sample.  Prints "ok" and exits 0, else the first failures.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fsk_resample_plan.h"

using namespace fsk;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (failures++ < 20) { std::printf("line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                           \
  } while (0)

// the owners of the next history's entries, as the kernels decide them: sample m (up: input, down: input t) staged by the
// workgroup of segment start m0 at position i of its staged span (the first `pad` positions lie in front of the segment)
static void walk_history(uint32_t H, uint32_t pad, size_t seg_inputs, size_t n_in, uint32_t L, uint32_t taps) {
  std::vector<int> written(H, 0);
  for (size_t m0 = 0; m0 < n_in; m0 += seg_inputs) {
    for (size_t i = 0; i < pad + seg_inputs; i++) {
      const int64_t m = (int64_t)m0 + (int64_t)i - (int64_t)pad;
      const int64_t h = m + (int64_t)H - (int64_t)n_in;
      if (m < -(int64_t)H) continue;                              // (down: in front of the history, staged as 0 and never read)
      if ((i >= pad || m0 == 0) && h >= 0 && m < (int64_t)n_in) {
        CHECK(h < (int64_t)H, "L %u taps %u n %zu", L, taps, n_in);
        if (h < (int64_t)H) written[(size_t)h]++;
      }
    }
  }
  for (uint32_t h = 0; h < H; h++) CHECK(written[h] == 1, "history %u written %d times (L %u taps %u n %zu)", h, written[h], L, taps, n_in);
}

int main() {
  for (uint32_t L = 1; L <= kResampleMaxFactor; L++) {
    for (uint32_t taps = 1; taps <= kResampleMaxTaps; taps++) {
      const uint32_t K = resample_phase_len(L, taps), Hu = resample_history(0, L, taps), Hd = resample_history(1, L, taps);
      CHECK(Hu + 1 >= K && (uint64_t)Hu * L >= taps - 1 && (uint64_t)(Hu ? Hu - 1 : 0) * L < taps, "L %u taps %u", L, taps);
      CHECK(Hd == taps - 1, "L %u taps %u", L, taps);
      if (taps <= 200 || taps % 97 == 0 || taps == kResampleMaxTaps) {
        uint32_t sum = 0;
        for (uint32_t p = 0; p < L; p++) {
          const uint32_t kp = resample_phase_taps(L, taps, p);
          CHECK(kp <= K && kp == taps / L + (p < taps % L ? 1u : 0u), "L %u taps %u p %u", L, taps, p);
          sum += kp;
        }
        CHECK(sum == taps, "L %u taps %u", L, taps);
      }
      for (int rows = 0; rows < 2; rows++) {
        for (size_t n : {(size_t)1, (size_t)63, (size_t)1025, (size_t)8000}) {
          const uint32_t S = 130;
          const ResamplePlan U = resample_up_plan(rows, L, taps, S, n);
          const uint32_t ns = 1u << U.log2_ns;
          CHECK(U.lds_bytes <= kResampleLdsBytes && U.hist == Hu && U.x_pitch >= U.hist + U.seg && U.seg % 64 == 0, "up L %u taps %u", L, taps);
          CHECK(U.lds_bytes == 4ull * ((size_t)ns * U.x_pitch + 256ull * L), "up L %u taps %u", L, taps);
          CHECK(rows ? ns == 1 : ns <= 64, "up L %u taps %u", L, taps);
          CHECK(U.blocks == (rows ? (uint64_t)S : (uint64_t)(S + ns - 1) / ns) * ((n + U.seg - 1) / U.seg) && U.split > 0, "up L %u taps %u", L, taps);
          const size_t n_out = n;   // outputs per stream of a down call
          const ResamplePlan D = resample_down_plan(rows, L, taps, S, n_out);
          const uint32_t nd = 1u << D.log2_ns;
          CHECK(D.lds_bytes <= kResampleLdsBytes && D.hist == Hd && D.hist_pad % L == 0 && D.hist_pad >= Hd && D.hist_pad < Hd + L, "down L %u taps %u", L, taps);
          CHECK(D.seg % 64 == 0 && D.seg >= 64 && D.x_pitch == L * D.q_len && D.q_len == D.hist_pad / L + D.seg, "down L %u taps %u", L, taps);
          CHECK(D.lds_bytes == 4ull * ((size_t)nd * D.x_pitch + (rows ? 0u : 64u * (nd + 1u))), "down L %u taps %u", L, taps);
          // the furthest word a lane reads: output seg - 1, tap 0 -> input (seg - 1) L + hist_pad, at [0][seg - 1 + hist_pad / L]
          CHECK((uint64_t)(D.seg - 1) * L + D.hist_pad < D.x_pitch, "down L %u taps %u", L, taps);
          CHECK(D.blocks == (rows ? (uint64_t)S : (uint64_t)(S + nd - 1) / nd) * ((n_out + D.seg - 1) / D.seg), "down L %u taps %u", L, taps);
        }
      }
      if (taps <= 40 || taps == 97 || taps == kResampleMaxTaps) {
        for (size_t n : {(size_t)1, (size_t)3, (size_t)64, (size_t)65, (size_t)1030}) {
          for (int rows = 0; rows < 2; rows++) {
            const ResamplePlan U = resample_up_plan(rows, L, taps, 1, n);
            walk_history(U.hist, U.hist, U.seg, n, L, taps);
            const ResamplePlan D = resample_down_plan(rows, L, taps, 1, n);
            walk_history(D.hist, D.hist_pad, (size_t)D.seg * L, n * L, L, taps);
          }
        }
      }
    }
  }
  CHECK(resample_out_count(0, 6, 8000) == 48000 && resample_out_count(1, 6, 48000) == 8000, "counts");
  CHECK(resample_down_length(6, 97, 0) == 16 && resample_down_length(6, 97, 1) == 17 && resample_down_length(6, 97, 48000) == 8016, "lengths");
  CHECK(resample_up_plan(true, 1, 1, 0x7FFFFFFFu, (size_t)1 << 40).blocks == 0, "a grid past one launch");
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
