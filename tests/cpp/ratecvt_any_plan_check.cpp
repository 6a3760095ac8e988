// ratecvt_any_plan_check.cpp -- the arithmetic of the rate converter's calls of any length (webaudio_modem_amd/csrc/
// fsk_ratecvt_plan.h: "Calls of any length") from a program of its own, for a sanitizer run without a GPU.
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I webaudio_modem_amd/csrc
//     tests/cpp/ratecvt_any_plan_check.cpp -o ratecvt_any_plan_check && ./ratecvt_any_plan_check
// For every coprime L, M <= 12, and 160 / 147 and 147 / 160; every position pos < M; n = 1 .. 3 M + 1; tap counts 1, L, L + 1 and
// 16 max(L, M) + 1; both layouts:
//   * ratecvt_out_count_any summed over a cut equals the uncut count, whole periods from 0 give ratecvt_out_count, and the
//     position after the cut is the position after the whole;
//   * ratecvt_in_count_any is the smallest n_in that writes n_out, and writes exactly n_out where L <= M;
//   * walking the launch as ratecvt_body<ANY> cuts it: every output that it would evaluate reads staged indices x0 - k inside
//     [0, span) of its row and inside the call's inputs and the history in front of them, its newest input is input (jM) div L of
//     the grid; every output of the call is evaluated by exactly one workgroup, row and place, and every word of the next history
//     is written by exactly one workgroup, from the call's inputs or the old history.
// Prints "ok" and exits 0, else the first failures.
#include <cstdint>
#include <cstdio>
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

static size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

static void counts(uint32_t L, uint32_t M) {
  for (uint32_t pos = 0; pos < M; pos++) {
    CHECK(ratecvt_first_output(L, M, pos) == ceil_div((size_t)pos * L, M), "%u/%u pos %u", L, M, pos);
    CHECK(ratecvt_in_count_any(L, M, pos, 0) == 0 && ratecvt_out_count_any(L, M, pos, 0) == 0, "%u/%u pos %u", L, M, pos);
    for (size_t n = 1; n <= 3u * M + 1u; n++) {
      const size_t whole = ratecvt_out_count_any(L, M, pos, n);
      CHECK(whole == ceil_div((pos + n) * L, M) - ceil_div((size_t)pos * L, M), "%u/%u pos %u n %zu", L, M, pos, n);
      if (pos == 0 && n % M == 0) CHECK(whole == ratecvt_out_count(L, M, n), "%u/%u n %zu", L, M, n);
      // the outputs counted are those whose newest input lies in [pos, pos + n)
      size_t direct = 0;
      for (size_t j = 0; j * M / L < pos + n; j++) direct += j * M / L >= pos;
      CHECK(direct == whole, "%u/%u pos %u n %zu: %zu outputs have their newest input in the call, counted %zu", L, M, pos, n, direct, whole);
      // every cut in two, and a cut into ones
      for (size_t a = 0; a <= n; a++) {
        const uint32_t mid = ratecvt_next_position(M, pos, a);
        CHECK(ratecvt_out_count_any(L, M, pos, a) + ratecvt_out_count_any(L, M, mid, n - a) == whole, "%u/%u pos %u n %zu cut at %zu", L, M, pos, n, a);
        CHECK(ratecvt_next_position(M, mid, n - a) == ratecvt_next_position(M, pos, n), "%u/%u pos %u n %zu cut at %zu", L, M, pos, n, a);
      }
      size_t ones = 0;
      uint32_t at = pos;
      for (size_t t = 0; t < n; t++) { ones += ratecvt_out_count_any(L, M, at, 1); at = ratecvt_next_position(M, at, 1); }
      CHECK(ones == whole && at == (pos + n) % M, "%u/%u pos %u n %zu in ones", L, M, pos, n);
      // the inverse: the smallest n_in that writes at least n_out; exact where L <= M
      for (size_t n_out = 1; n_out <= whole + 1; n_out++) {
        const size_t need = ratecvt_in_count_any(L, M, pos, n_out);
        CHECK(need >= 1 && ratecvt_out_count_any(L, M, pos, need) >= n_out && ratecvt_out_count_any(L, M, pos, need - 1) < n_out, "%u/%u pos %u n_out %zu: %zu",
              L, M, pos, n_out, need);
        if (L <= M) CHECK(ratecvt_out_count_any(L, M, pos, need) == n_out, "%u/%u pos %u n_out %zu: %zu", L, M, pos, n_out, need);
      }
    }
  }
}

// one launch over one stream tile, workgroup by workgroup, as ratecvt_body<ANY> cuts it
static void walk(bool rows, bool playback, uint32_t L, uint32_t M, uint32_t taps, uint32_t pos, size_t n_in) {
  const uint32_t S = rows ? 1u : 3u;
  const RatecvtPlan P = ratecvt_plan(rows, playback, L, M, taps, S, pos, n_in);
  const uint32_t H = P.hist, ns = 1u << P.log2_ns, Qs = P.G * L, k_full = taps / L, rem = taps % L;
  const size_t j_lo = ratecvt_first_output(L, M, pos), j_hi = ratecvt_first_output(L, M, pos + n_in), n_out = ratecvt_out_count_any(L, M, pos, n_in);
  const size_t x_words = (size_t)ns * P.x_pitch, periods = ceil_div(pos + n_in, M);
  const uint64_t segs = rows ? P.split : P.blocks / P.split;
  CHECK(P.blocks == (rows ? segs * S : segs * ((S + ns - 1) / ns)) && segs * P.seg_periods >= periods && (segs - 1) * P.seg_periods < periods && j_hi - j_lo == n_out,
        "%u/%u taps %u pos %u n %zu", L, M, taps, pos, n_in);
  std::vector<int> out_written(n_out, 0), hist_written(H, 0);
  for (uint64_t seg = 0; seg < segs; seg++) {
    const size_t per0 = (size_t)seg * P.seg_periods, m0 = per0 * M, j0 = per0 * L;
    for (uint32_t i = 0; i < P.span; i++) {                         // stream c = 0 of the tile
      const int64_t m = (int64_t)m0 + (int64_t)i - (int64_t)H - (int64_t)pos, h = m + (int64_t)H - (int64_t)n_in;
      if ((i >= H || m0 == 0) && h >= 0 && m < (int64_t)n_in) {
        CHECK(h < (int64_t)H && m >= -(int64_t)H, "%u/%u taps %u pos %u n %zu", L, M, taps, pos, n_in);   // an input of the call or a word of the old history
        if (h < (int64_t)H) hist_written[(size_t)h]++;
      }
    }
    const uint32_t n_quads = (P.rows + 3) / 4;
    for (uint32_t quad = 0; quad < n_quads; quad++) {
      for (uint32_t r = 0; r < 4; r++) {
        const uint32_t row = quad * 4 + r;
        if (row >= P.rows || (!rows && row != 0)) continue;       // (sample-major: the rows are streams, alike)
        const size_t jr = j0 + (rows ? (size_t)row * Qs : 0);
        // the places the body evaluates are those with j_lo <= j < j_hi; every other place of the row is skipped.  (In a lane's
        // quad the body computes the lane's first own row again in a skipped row's stead: the same indices as that own row's,
        // which are walked here; sample-major the rows are streams with one set of indices at different bases, so row 0 stands
        // for all.)
        for (uint32_t u = 0; u < Qs && jr + u < j_hi; u++) {
          const size_t j = jr + u;
          if (j < j_lo) continue;
          const uint32_t per = u / L, q = u % L, word = ratecvt_table_word(L, M, q), p = word >> 16;
          const uint32_t x0 = H + per * M + (word & 0xFFFFu), kp = k_full + (p < rem ? 1u : 0u);
          const size_t base = (size_t)row * P.row_stride, hi = base + x0;
          CHECK(kp >= 1 ? x0 >= kp - 1 : true, "%u/%u taps %u u %u", L, M, taps, u);
          const size_t lo = hi - (kp ? kp - 1 : 0);
          CHECK(hi < x_words && lo >= base && (rows ? hi < P.span : x0 < P.span), "%u/%u taps %u pos %u n %zu row %u u %u", L, M, taps, pos, n_in, row, u);
          // on the grid: the newest input is (jM) div L, inside the call; the oldest no further back than the history
          const size_t newest = m0 + (rows ? base : 0) + (x0 - H);
          CHECK(newest == j * M / L && newest >= pos && newest < pos + n_in && newest + H >= pos + (kp ? kp - 1 : 0), "%u/%u taps %u pos %u n %zu j %zu", L, M, taps, pos,
                n_in, j);
          if (!rows && playback) CHECK(x_words + (size_t)u * (ns + 1) + row < P.lds_bytes / 4, "%u/%u taps %u", L, M, taps);
          out_written[j - j_lo]++;
        }
      }
    }
  }
  for (size_t j = 0; j < n_out; j++) CHECK(out_written[j] == 1, "output %zu evaluated %d times (%u/%u taps %u pos %u n %zu rows %d)", j, out_written[j], L, M, taps, pos, n_in, rows);
  for (uint32_t h = 0; h < H; h++) CHECK(hist_written[h] == 1, "history %u written %d times (%u/%u taps %u pos %u n %zu rows %d)", h, hist_written[h], L, M, taps, pos, n_in, rows);
}

static void ratio(uint32_t L, uint32_t M) {
  counts(L, M);
  for (const uint32_t taps : {1u, L, L + 1u, 16u * (L > M ? L : M) + 1u}) {
    for (int rows = 0; rows < 2; rows++) {
      // a whole-period launch from 0 is the plan the whole-period kernels take: the shape's grid over n_in / M periods
      const RatecvtPlan A = ratecvt_plan(rows, true, L, M, taps, 5, 0, (size_t)7 * M);
      RatecvtPlan B = ratecvt_shape(rows, true, L, M, taps);
      resample_grid(B, B.seg_periods, rows, 5, 7);
      CHECK(A.blocks == B.blocks && A.split == B.split && A.span == B.span && A.lds_bytes == B.lds_bytes && A.G == B.G, "%u/%u taps %u", L, M, taps);
      for (uint32_t pos = 0; pos < M; pos++)
        for (size_t n = 1; n <= 3u * M + 1u; n++) walk(rows, rows == 0 && ((pos + n) & 1u), L, M, taps, pos, n);
      // past one workgroup and past two, from the last position
      const size_t seg_in = (size_t)A.seg_periods * M;
      for (const size_t n : {seg_in, seg_in + 1, 2 * seg_in + M / 2 + 1}) walk(rows, !rows, L, M, taps, M - 1, n);
    }
  }
}

int main() {
  for (uint32_t L = 1; L <= 12; L++)
    for (uint32_t M = 1; M <= 12; M++)
      if (ratecvt_gcd(L, M) == 1) ratio(L, M);
  ratio(160, 147);
  ratio(147, 160);
  // 13 of the 160 positions of 147 / 160 write nothing for one input, and one period from anywhere writes L
  uint32_t none = 0;
  for (uint32_t pos = 0; pos < 160; pos++) {
    none += ratecvt_out_count_any(147, 160, pos, 1) == 0;
    CHECK(ratecvt_out_count_any(147, 160, pos, 160) == 147 && ratecvt_out_count_any(147, 160, pos, 480) == 441, "pos %u", pos);
  }
  CHECK(none == 13, "%u positions of 147 / 160 write nothing", none);
  CHECK(ratecvt_out_count_any(160, 147, 0, 128) == 140 && ratecvt_out_count_any(160, 147, 128, 128) == 139 && ratecvt_in_count_any(147, 160, 0, 128) == 139, "a 128-frame quantum");
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
