// processor_ratecvt_plan_check.cpp -- how fskhip_processor_process_ratecvt_* chooses between its fused TX kernel and the two
// launches it replaces (webaudio_modem_amd/csrc/fsk_processor_rate_plan.h: processor_ratecvt_plan), from a program of its own, for a
// sanitizer run without a GPU.
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I webaudio_modem_amd/csrc
//     tests/cpp/processor_ratecvt_plan_check.cpp -o processor_ratecvt_plan_check && ./processor_ratecvt_plan_check
// Checked, for up factors 1..256, tap counts 1..4096, every element size and both layouts: the delay line is the handle's history
// (fsk_ratecvt_plan.h's, H = ceil((n_taps - 1) / L)) and the generator's step; a plan's LDS is the delay line plus the code rows;
// it is fused exactly where that is within the budget and the layout is stream-major; the fallback starts exactly where the budget
// ends; 147 / 160 with 2 561 taps fits with 22 slots (under 6 KB of delay line) and 160 / 147 too; L = 1 with 4 096 taps does not
// fit.  And by walking the kernel's ring of slots with its two accumulators, for ratios either side of 1 and quanta down to one
// period of fewer engine samples than H: every output is taken exactly once, in order, when its newest input has just been written,
// every product reads the sample the converter's formula names, and the history left is the last H samples -- old ones among them
// where the quantum was shorter.  Prints "ok" and exits 0.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fsk_processor_rate_plan.h"
#include "fsk_ratecvt_plan.h"

using namespace fsk;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (failures++ < 20) { std::printf("line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                           \
  } while (0)

// the kernel's walk over a quantum of `periods` periods: slot -> the sample it holds (history sample -H + h is h - H)
static void walk_ring(uint32_t L, uint32_t M, uint32_t taps, uint32_t slots, size_t periods) {
  const int64_t H = resample_history(0, L, taps), none = INT64_MIN;
  const uint32_t k_full = taps / L, rem = taps - k_full * L;
  std::vector<int64_t> held(slots, none);
  for (int64_t h = 0; h < H; h++) held[(size_t)h] = h - H;
  const size_t n_out = periods * L, n_high = periods * M;
  uint32_t wslot = (uint32_t)H, q = 0, ph = 0;
  size_t k = 0, m = 0;
  CHECK(wslot < slots, "L %u M %u taps %u", L, M, taps);
  for (size_t t0 = 0; t0 < n_high; t0 += kRateChunk) {
    const uint32_t cnt = n_high - t0 < kRateChunk ? (uint32_t)(n_high - t0) : kRateChunk;
    uint32_t sl = wslot;
    for (uint32_t j = 0; j < cnt; j++) { held[sl] = (int64_t)(t0 + j); sl = sl + 1 == slots ? 0 : sl + 1; }
    while (k < n_out && m < t0 + cnt) {
      CHECK(m >= t0, "L %u M %u taps %u output %zu was due before this step", L, M, taps, k);
      CHECK(m == k * M / L && ph == k * M % L && q == k % L, "L %u M %u output %zu: m %zu phase %u place %u", L, M, k, m, ph, q);
      CHECK(ratecvt_phase(L, M, q) == ph, "L %u M %u place %u", L, M, q);   // (column q of the table holds this phase)
      uint32_t si = wslot + (uint32_t)(m - t0);
      si = si >= slots ? si - slots : si;
      const uint32_t n_prod = k_full + (ph < rem ? 1u : 0u);
      CHECK(n_prod == resample_phase_taps(L, taps, ph), "L %u taps %u phase %u", L, taps, ph);
      for (uint32_t i = 0; i < n_prod; i++) {
        CHECK(held[si] == (int64_t)m - (int64_t)i, "L %u M %u taps %u periods %zu output %zu product %u reads sample %lld", L, M, taps, periods, k, i, (long long)held[si]);
        si = si == 0 ? slots - 1 : si - 1;
      }
      k++;
      q = q + 1 == L ? 0 : q + 1;
      ph += M;
      while (ph >= L) { ph -= L; m++; }
    }
    wslot = sl;
  }
  CHECK(k == n_out, "L %u M %u taps %u periods %zu: %zu outputs", L, M, taps, periods, k);
  const uint32_t hbase = (uint32_t)(n_high % slots);
  for (int64_t h = 0; h < H; h++) {
    uint32_t si = hbase + (uint32_t)h;
    si = si >= slots ? si - slots : si;
    CHECK(held[si] == (int64_t)n_high - H + h, "L %u M %u taps %u periods %zu history %lld holds sample %lld", L, M, taps, periods, (long long)h, (long long)held[si]);
  }
}

int main() {
  for (uint32_t L = 1; L <= kRatecvtMaxFactor; L++) {
    for (uint32_t esz : {1u, 2u, 4u}) {
      for (int rows = 0; rows < 2; rows++) {
        uint32_t first_unfit = 0;
        for (uint32_t taps = 1; taps <= kResampleMaxTaps; taps++) {
          const RatePlan P = processor_ratecvt_plan(L, taps, esz, rows != 0);
          CHECK(P.slots == resample_history(0, L, taps) + kRateChunk, "L %u taps %u", L, taps);
          CHECK(P.slots >= resample_phase_len(L, taps) - 1u + kRateChunk, "L %u taps %u", L, taps);   // (a sum reaches back K - 1)
          CHECK(P.code_words == 64u * (kRateCodeTile * esz / 4u + 1u), "L %u taps %u", L, taps);
          CHECK(P.lds_bytes == 4ull * ((uint64_t)P.slots * kRateLanePitch + P.code_words), "L %u taps %u", L, taps);
          CHECK(P.fits == (P.lds_bytes <= kRateLdsBytes), "L %u taps %u: %zu bytes", L, taps, P.lds_bytes);
          CHECK(P.fused == (P.fits && rows), "L %u taps %u", L, taps);
          if (!P.fits && !first_unfit) first_unfit = taps;
          CHECK(!first_unfit || !P.fits, "L %u taps %u fits behind %u that does not", L, taps, first_unfit);   // (one threshold)
        }
        // the boundary either side of the budget: the last plan that fits is within it, the next slot is not
        if (first_unfit) {
          const RatePlan A = processor_ratecvt_plan(L, first_unfit - 1, esz, rows != 0), B = processor_ratecvt_plan(L, first_unfit, esz, rows != 0);
          CHECK(first_unfit > 1 && A.lds_bytes <= kRateLdsBytes && B.lds_bytes > kRateLdsBytes, "L %u esz %u rows %d", L, esz, rows);
          CHECK(B.slots == A.slots + 1 && B.lds_bytes - A.lds_bytes == 4u * kRateLanePitch, "L %u esz %u rows %d", L, esz, rows);
          CHECK(A.fused == (rows != 0) && !B.fused, "L %u esz %u rows %d", L, esz, rows);
        } else {
          CHECK(processor_ratecvt_plan(L, kResampleMaxTaps, esz, rows != 0).fits, "L %u esz %u rows %d", L, esz, rows);
        }
      }
    }
  }
  // the designs the feature is for, and the one the fallback is tested with
  for (uint32_t esz : {1u, 2u, 4u}) {
    const RatePlan P = processor_ratecvt_plan(147, 2561, esz, true);
    CHECK(P.fits && P.fused && P.slots == 22 && 4u * P.slots * kRateLanePitch < 6144, "147 / 160, esz %u: %u slots", esz, P.slots);
    CHECK(!processor_ratecvt_plan(147, 2561, esz, false).fused, "frames take the pair");
    CHECK(processor_ratecvt_plan(160, 2561, esz, true).fused, "160 / 147, esz %u", esz);
    const RatePlan Q = processor_ratecvt_plan(1, 4096, esz, true);
    CHECK(!Q.fits && !Q.fused && Q.slots == 4099, "L 1, 4096 taps, esz %u: %u slots", esz, Q.slots);
  }
  const uint32_t ratios[][2] = {{3, 2}, {2, 3}, {1, 1}, {1, 4}, {5, 1}, {7, 5}, {5, 7}, {147, 160}, {160, 147}, {256, 255}, {1, 256}, {256, 1}};
  for (const auto &r : ratios) {
    for (uint32_t taps : {1u, 2u, 7u, 8u, 13u, 113u, 2561u}) {
      const RatePlan P = processor_ratecvt_plan(r[0], taps, 1, false);
      for (size_t periods : {(size_t)1, (size_t)2, (size_t)3, (size_t)12}) walk_ring(r[0], r[1], taps, P.slots, periods);
    }
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
