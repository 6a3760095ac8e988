// processor_rate_plan_check.cpp -- how fskhip_processor_process_rate_* chooses between its fused TX kernel and the two launches it
// replaces (webaudio_modem_amd/csrc/fsk_processor_rate_plan.h), from a program of its own, for a sanitizer run without a GPU: every
// factor 1..32 x every tap count 1..4096 x every element size x both layouts.
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I webaudio_modem_amd/csrc
//     tests/cpp/processor_rate_plan_check.cpp -o processor_rate_plan_check && ./processor_rate_plan_check
// Checked: a fused plan's LDS is within the budget and is the delay line plus the code rows; the delay line holds the history an
// output reaches back to and a factor's worth of new samples (and the generator's step); the default designs (16 L + 1 taps) fit
// up to L = 12 and are fused where the layout is stream-major (interleaved frames take the pair, which measured faster); the
// fallback starts exactly where the budget ends; and, by walking the kernel's ring of slots, that no sample
// is overwritten before the last output or the next history that needs it has read it.  Prints "ok" and exits 0.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fsk_processor_rate_plan.h"

using namespace fsk;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (failures++ < 20) { std::printf("line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                           \
  } while (0)

// the kernel's walk over a quantum of n_out outputs: slot -> the sample it holds (history sample -H + h is h - H)
static void walk_ring(uint32_t L, uint32_t taps, uint32_t slots, size_t n_out) {
  const int64_t H = taps - 1, none = INT64_MIN;
  std::vector<int64_t> held(slots, none);
  for (int64_t h = 0; h < H; h++) held[(size_t)h] = h - H;
  const size_t n_high = n_out * L;
  uint32_t wslot = (uint32_t)H, ph = 0;
  size_t k = 0;
  CHECK(wslot < slots, "L %u taps %u", L, taps);
  for (size_t t0 = 0; t0 < n_high; t0 += kRateChunk) {
    const uint32_t cnt = n_high - t0 < kRateChunk ? (uint32_t)(n_high - t0) : kRateChunk;
    uint32_t sl = wslot;
    for (uint32_t j = 0; j < cnt; j++) { held[sl] = (int64_t)(t0 + j); sl = sl + 1 == slots ? 0 : sl + 1; }
    for (uint32_t j = 0; j < cnt; j++) {
      if (ph == 0) {
        uint32_t si = wslot + j;
        si = si >= slots ? si - slots : si;
        for (uint32_t i = 0; i < taps; i++) {
          CHECK(held[si] == (int64_t)(k * L) - (int64_t)i, "L %u taps %u n_out %zu output %zu tap %u reads sample %lld", L, taps, n_out, k, i, (long long)held[si]);
          si = si == 0 ? slots - 1 : si - 1;
        }
        k++;
      }
      ph = ph + 1 == L ? 0 : ph + 1;
    }
    wslot = sl;
  }
  CHECK(k == n_out, "L %u taps %u n_out %zu: %zu outputs", L, taps, n_out, k);
  const uint32_t hbase = (uint32_t)(n_high % slots);
  for (int64_t h = 0; h < H; h++) {
    uint32_t si = hbase + (uint32_t)h;
    si = si >= slots ? si - slots : si;
    CHECK(held[si] == (int64_t)n_high - H + h, "L %u taps %u n_out %zu history %lld holds sample %lld", L, taps, n_out, (long long)h, (long long)held[si]);
  }
}

int main() {
  for (uint32_t L = 1; L <= 32; L++) {
    for (uint32_t esz : {1u, 2u, 4u}) {
      for (int rows = 0; rows < 2; rows++) {
        uint32_t first_unfused = 0;
        for (uint32_t taps = 1; taps <= 4096; taps++) {
          const RatePlan P = processor_rate_plan(L, taps, esz, rows != 0);
          CHECK(P.slots >= taps - 1 + L && P.slots >= taps - 1 + kRateChunk, "L %u taps %u", L, taps);
          CHECK(P.code_words == 64u * (kRateCodeTile * esz / 4u + 1u), "L %u taps %u", L, taps);
          CHECK(P.lds_bytes == 4ull * ((uint64_t)P.slots * kRateLanePitch + P.code_words), "L %u taps %u", L, taps);
          CHECK(P.fits == (P.lds_bytes <= kRateLdsBytes), "L %u taps %u: %zu bytes", L, taps, P.lds_bytes);
          CHECK(P.fused == (P.fits && rows), "L %u taps %u", L, taps);   // (interleaved frames take the pair: it measured faster)
          if (!P.fits && !first_unfused) first_unfused = taps;
          CHECK(!first_unfused || !P.fits, "L %u taps %u fits behind %u that does not", L, taps, first_unfused);   // (one threshold)
        }
        // the fallback starts exactly where the budget ends: the last fused filter fits, one tap more does not
        CHECK(first_unfused > 1, "L %u esz %u rows %d", L, esz, rows);
        if (first_unfused > 1) {
          CHECK(processor_rate_plan(L, first_unfused - 1, esz, rows != 0).lds_bytes <= kRateLdsBytes, "L %u esz %u rows %d", L, esz, rows);
          CHECK(processor_rate_plan(L, first_unfused, esz, rows != 0).lds_bytes > kRateLdsBytes, "L %u esz %u rows %d", L, esz, rows);
          CHECK(processor_rate_plan(L, first_unfused, esz, rows != 0).lds_bytes - processor_rate_plan(L, first_unfused - 1, esz, rows != 0).lds_bytes ==
                    4u * kRateLanePitch, "L %u esz %u rows %d", L, esz, rows);
        }
        if (L <= 12) CHECK(processor_rate_plan(L, 16 * L + 1, esz, rows != 0).fits, "the default design of L %u (esz %u rows %d) does not fit", L, esz, rows);
        if (L <= 12 && rows) CHECK(processor_rate_plan(L, 16 * L + 1, esz, true).fused, "the default design of L %u (esz %u) is not fused", L, esz);
      }
    }
    for (uint32_t taps = 1; taps <= 4096; taps = taps < 40 ? taps + 1 : taps * 2 + 1) {
      const RatePlan P = processor_rate_plan(L, taps, 1, false);
      for (size_t n_out : {(size_t)1, (size_t)3, (size_t)37, (size_t)160}) walk_ring(L, taps, P.slots, n_out);
    }
    walk_ring(L, 16 * L + 1, processor_rate_plan(L, 16 * L + 1, 1, false).slots, 160);
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
