// ratecvt_plan_check.cpp -- the rational rate converter's host arithmetic (webaudio_modem_amd/csrc/fsk_ratecvt_plan.h) from a
// program of its own, for a sanitizer run without a GPU.
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I webaudio_modem_amd/csrc
//     tests/cpp/ratecvt_plan_check.cpp -o ratecvt_plan_check && ./ratecvt_plan_check
// Checked, for the ratios 160/147, 147/160, 3/2, 2/3, 7/5, 1/1, 256/255 and 1/256 and tap counts 1, L - 1, L and 16 max(L, M) + 1
// (where that is at most 4096), both layouts and both directions: the period table visits every phase exactly once, its offsets
// are monotone and end at M; the history is at least the longest phase minus one; a workgroup's LDS fits and holds every index the
// kernels form; and, by walking the workgroups as the kernels do, that every output and every word of the next history is owned
// by exactly one of them.  Prints "ok" and exits 0, else the first failures.  With the argument "table" it prints the plan's
// periods per workgroup instead (below).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "fsk_ratecvt_plan.h"

using namespace fsk;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (failures++ < 20) { std::printf("line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                           \
  } while (0)

// one launch over one stream tile, workgroup by workgroup, as ratecvt_body cuts it: who writes which output, which history word,
// and the LDS words it touches
static void walk(bool rows, bool playback, uint32_t L, uint32_t M, uint32_t taps, size_t n_in) {
  const uint32_t S = rows ? 1u : 3u;
  const RatecvtPlan P = ratecvt_plan(rows, playback, L, M, taps, S, 0, n_in);
  const uint32_t H = P.hist, ns = 1u << P.log2_ns, Qs = P.G * L, k_full = taps / L, rem = taps % L;
  const size_t n_out = ratecvt_out_count(L, M, n_in), x_words = (size_t)ns * P.x_pitch, lds_words = P.lds_bytes / 4;
  const uint64_t segs = rows ? P.split : P.blocks / P.split;
  CHECK(P.blocks == (rows ? segs * S : segs * ((S + ns - 1) / ns)) && segs * P.seg_periods * M >= n_in && (segs - 1) * P.seg_periods * M < n_in,
        "%u/%u taps %u n %zu", L, M, taps, n_in);
  std::vector<int> out_written(n_out, 0), hist_written(H, 0);
  for (uint64_t seg = 0; seg < segs; seg++) {
    const size_t per0 = (size_t)seg * P.seg_periods, m0 = per0 * M, j0 = per0 * L;
    for (uint32_t i = 0; i < P.span; i++) {                         // stream c = 0 of the tile
      CHECK(i < P.x_pitch, "%u/%u taps %u", L, M, taps);
      const int64_t m = (int64_t)m0 + (int64_t)i - (int64_t)H, h = m + (int64_t)H - (int64_t)n_in;
      if ((i >= H || m0 == 0) && h >= 0 && m < (int64_t)n_in) {
        CHECK(h < (int64_t)H, "%u/%u taps %u n %zu", L, M, taps, n_in);
        if (h < (int64_t)H) hist_written[(size_t)h]++;
      }
    }
    const uint32_t n_quads = (P.rows + 3) / 4;
    for (uint32_t w = 0; w < n_quads * Qs; w++) {
      const uint32_t quad = w / Qs, u = w % Qs, per = u / L, q = u % L, word = ratecvt_table_word(L, M, q), p = word >> 16;
      const uint32_t x0 = H + per * M + (word & 0xFFFFu), kp = k_full + (p < rem ? 1u : 0u);
      CHECK(kp == resample_phase_taps(L, taps, p) && (kp == 0 || kp - 1 <= H), "%u/%u taps %u p %u", L, M, taps, p);
      for (uint32_t r = 0; r < 4; r++) {
        const uint32_t row = quad * 4 + r;
        if (row >= P.rows) continue;
        const size_t hi = (size_t)row * P.row_stride + x0, lo = hi - (kp ? kp - 1 : 0);
        CHECK(hi < x_words && lo >= (size_t)row * P.row_stride && (rows || hi < (size_t)(row + 1) * P.x_pitch), "%u/%u taps %u row %u u %u", L, M, taps, row, u);
        const size_t j = j0 + (rows ? (size_t)row * Qs : 0) + u;
        if (!rows && playback) CHECK(x_words + (size_t)u * (ns + 1) + row < lds_words, "%u/%u taps %u", L, M, taps);
        if (j < n_out && (rows || row == 0)) {
          // the newest input the output reads is input (jM) div L of the stream
          CHECK(m0 + (rows ? (size_t)row * P.row_stride : 0) + (x0 - H) == j * M / L, "%u/%u taps %u j %zu", L, M, taps, j);
          out_written[j]++;
        }
      }
    }
  }
  for (size_t j = 0; j < n_out; j++) CHECK(out_written[j] == 1, "output %zu written %d times (%u/%u taps %u n %zu rows %d)", j, out_written[j], L, M, taps, n_in, rows);
  for (uint32_t h = 0; h < H; h++) CHECK(hist_written[h] == 1, "history %u written %d times (%u/%u taps %u n %zu rows %d)", h, hist_written[h], L, M, taps, n_in, rows);
}

// "table": the periods per workgroup of every shape the GPU tests walk, one line "L M n_taps playback stream-major sample-major" each,
// for tests/test_ratecvt_cpu.py to hold the GPU tests' own arithmetic (tests/test_gpu_ratecvt.py: _seg_periods) against this header
static int table() {
  const uint32_t pairs[][2] = {{3, 2}, {2, 3}, {7, 5}, {1, 1}, {160, 147}, {147, 160}};
  for (const auto &pr : pairs) {
    const uint32_t L = pr[0], M = pr[1];
    for (const uint32_t taps : {1u, 5u, L > 1 ? L - 1 : 1u, 13u, 16 * (L > M ? L : M) + 1})
      for (int playback = 0; playback < 2; playback++)
        std::printf("%u %u %u %d %u %u\n", L, M, taps, playback, ratecvt_plan(true, playback, L, M, taps, 1, 0, M).seg_periods,
                    ratecvt_plan(false, playback, L, M, taps, 1, 0, M).seg_periods);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::string(argv[1]) == "table") return table();
  const uint32_t pairs[][2] = {{160, 147}, {147, 160}, {3, 2}, {2, 3}, {7, 5}, {1, 1}, {256, 255}, {1, 256}};
  for (const auto &pr : pairs) {
    const uint32_t L = pr[0], M = pr[1];
    CHECK(ratecvt_gcd(L, M) == 1, "%u/%u", L, M);
    std::vector<int> seen(L, 0);
    uint32_t last = 0;
    for (uint32_t q = 0; q < L; q++) {
      const uint32_t p = ratecvt_phase(L, M, q), off = ratecvt_offset(L, M, q);
      CHECK(p < L && (uint64_t)off * L + p == (uint64_t)q * M && off >= last && off < M, "%u/%u q %u", L, M, q);
      CHECK(ratecvt_table_word(L, M, q) == (off | p << 16), "%u/%u q %u", L, M, q);
      if (p < L) seen[p]++;
      last = off;
    }
    for (uint32_t p = 0; p < L; p++) CHECK(seen[p] == 1, "%u/%u phase %u met %d times", L, M, p, seen[p]);
    CHECK(ratecvt_offset(L, M, L) == M && ratecvt_phase(L, M, L) == 0, "%u/%u: a period is M inputs", L, M);
    std::vector<uint32_t> tap_counts = {1u, L > 1 ? L - 1 : 1u, L};
    if (16 * (L > M ? L : M) + 1 <= kResampleMaxTaps) tap_counts.push_back(16 * (L > M ? L : M) + 1);
    tap_counts.push_back(kResampleMaxTaps);
    for (const uint32_t taps : tap_counts) {
      const uint32_t K = resample_phase_len(L, taps), H = resample_history(0, L, taps);
      uint32_t sum = 0, longest = 0;
      for (uint32_t p = 0; p < L; p++) {
        const uint32_t kp = resample_phase_taps(L, taps, p);
        sum += kp;
        longest = kp > longest ? kp : longest;
      }
      CHECK(sum == taps && longest == K && H + 1 >= K && (uint64_t)H * L >= taps - 1 && (uint64_t)(H ? H - 1 : 0) * L < taps, "%u/%u taps %u", L, M, taps);
      for (int rows = 0; rows < 2; rows++) {
        for (int playback = 0; playback < 2; playback++) {
          const RatecvtPlan P = ratecvt_plan(rows, playback, L, M, taps, 130, 0, (size_t)M);
          const uint32_t ns = 1u << P.log2_ns;
          CHECK(P.lds_bytes <= kResampleLdsBytes && P.hist == H && P.G >= 1 && P.span == H + P.seg_periods * M && P.x_pitch >= P.span, "%u/%u taps %u", L, M, taps);
          CHECK(rows ? (ns == 1 && P.rows == 4 && P.seg_periods == 4 * P.G && P.row_stride == P.G * M && P.lds_bytes == 4ull * P.span)
                     : (ns <= 64 && P.rows == ns && P.seg_periods == P.G && P.row_stride == P.x_pitch && (P.x_pitch & 1u) &&
                        P.lds_bytes == 4ull * ((size_t)ns * P.x_pitch + P.tile_words) && P.tile_words == (playback ? P.G * L * (ns + 1) : 0u)),
                "%u/%u taps %u rows %d", L, M, taps, rows);
          // n_in of M, 3 M and one length on each side of the plan's own segment boundary
          const size_t seg_in = (size_t)P.seg_periods * M;
          for (const size_t n_in : {(size_t)M, (size_t)3 * M, seg_in, seg_in + M, seg_in > M ? seg_in - M : (size_t)M, 2 * seg_in + M}) walk(rows, playback, L, M, taps, n_in);
        }
      }
    }
  }
  CHECK(ratecvt_out_count(160, 147, 44100) == 48000 && ratecvt_out_count(147, 160, 48000) == 44100, "counts");
  CHECK(ratecvt_out_length(147, 160, 2561, 0) == 0 && ratecvt_out_length(147, 160, 2561, 1) == 17 && ratecvt_out_length(1, 1, 1, 5) == 5 &&
            ratecvt_out_length(6, 1, 97, 10) == 151 && ratecvt_out_length(1, 6, 97, 48000) == 8016,
        "lengths");
  CHECK(resample_history(0, 160, 2561) == 16 && resample_history(0, 147, 2561) == 18 && resample_history(0, 1, 1) == 0, "histories");
  CHECK(ratecvt_plan(true, false, 1, 1, 1, 0x7FFFFFFFu, 0, (size_t)1 << 40).blocks == 0, "a grid past one launch");
  CHECK(ratecvt_plan(false, true, 1, 1, 1, 64, 0, (size_t)1 << 40).blocks == 0, "a grid past one launch");
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
