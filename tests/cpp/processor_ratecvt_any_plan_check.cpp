// processor_ratecvt_any_plan_check.cpp -- where the any-length form of the fused TX kernel starts
// (webaudio_modem_amd/csrc/fsk_processor_rate_plan.h: processor_ratecvt_start, processor_ratecvt_any), from a program of its own, for a
// sanitizer run without a GPU.
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I webaudio_modem_amd/csrc
//     tests/cpp/processor_ratecvt_any_plan_check.cpp -o processor_ratecvt_any_plan_check && ./processor_ratecvt_any_plan_check
// For (L, M) = (147, 160), (160, 147), (3, 2), (2, 3), (1, 6), (6, 1), (1, 1), (255, 256), every position 0 .. M - 1 and n_out in
// {1, 2, L - 1, L, L + 1, 128, 129}: k0, q, ph and m against brute force -- the grid's outputs enumerated from the boundary, the first
// whose newest input is >= pos --; n_high is ratecvt_in_count_any; the last output's newest input is < n_high; the position after the
// call is ratecvt_next_position; and which form the launcher picks.  Then the kernel's walk over its ring of slots from that start,
// call after call from where the last one left off: every output the call can write is taken once, in order, as soon as its newest
// input is written, every product reads the sample the converter's formula names, and the history left is the H newest samples --
// old ones among them where the call was shorter than H.  Prints "ok" and exits 0.
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

static void check_start(uint32_t L, uint32_t M, uint32_t pos, size_t n_out) {
  const RatecvtStart s = processor_ratecvt_start(L, M, pos, n_out);
  size_t j = 0;                                   // brute force: the first output of the grid whose newest input lies in the call
  while (j * M / L < pos) j++;
  CHECK(s.k0 == j, "L %u M %u pos %u: k0 %zu, brute force %zu", L, M, pos, s.k0, j);
  CHECK(s.q == j % L && s.ph == j * M % L && s.m == j * M / L - pos, "L %u M %u pos %u: q %u ph %u m %u", L, M, pos, s.q, s.ph, s.m);
  CHECK(s.q < L && s.ph < L && ratecvt_phase(L, M, s.q) == s.ph, "L %u M %u pos %u: column %u holds phase %u", L, M, pos, s.q, s.ph);
  CHECK(s.n_high == ratecvt_in_count_any(L, M, pos, n_out), "L %u M %u pos %u n_out %zu", L, M, pos, n_out);
  const size_t last = (j + n_out - 1) * M / L - pos;     // the last output's newest input, from the call's first sample
  CHECK(last < s.n_high && last + 1 == s.n_high, "L %u M %u pos %u n_out %zu: last input %zu of %zu", L, M, pos, n_out, last, s.n_high);
  CHECK(ratecvt_next_position(M, pos, s.n_high) == (pos + s.n_high) % M, "L %u M %u pos %u", L, M, pos);
  // whole periods of both rates from a boundary are the other form's
  CHECK(processor_ratecvt_any(L, M, pos, n_out, s.n_high) == !(pos == 0 && n_out % L == 0 && s.n_high == n_out / L * M), "L %u M %u pos %u n_out %zu", L, M, pos, n_out);
  CHECK(!processor_ratecvt_any(L, M, 0, n_out * L, n_out * M) && processor_ratecvt_any(L, M, 0, n_out * L, n_out * M + 1), "L %u M %u", L, M);
}

// the kernel's walk over one call from `pos`; `held`: slot -> the sample of the stream it holds, counted from the stream's first
// (history sample -H + h of the call is base - H + h); returns the samples the call took, or 0 for a count the position cannot write
static size_t walk_call(uint32_t L, uint32_t M, uint32_t taps, uint32_t slots, uint32_t pos, size_t n_out, int64_t base, std::vector<int64_t> &ring_hist) {
  const int64_t H = resample_history(0, L, taps);
  const uint32_t k_full = taps / L, rem = taps - k_full * L;
  const RatecvtStart s = processor_ratecvt_start(L, M, pos, n_out);
  if (ratecvt_out_count_any(L, M, pos, s.n_high) != n_out) return 0;
  std::vector<int64_t> held(slots, INT64_MIN);
  for (int64_t h = 0; h < H; h++) held[(size_t)h] = ring_hist[(size_t)h];
  const size_t n_high = s.n_high;
  uint32_t wslot = (uint32_t)H, q = s.q, ph = s.ph;
  size_t k = 0, m = s.m;
  for (size_t t0 = 0; t0 < n_high; t0 += kRateChunk) {
    const uint32_t cnt = n_high - t0 < kRateChunk ? (uint32_t)(n_high - t0) : kRateChunk;
    uint32_t sl = wslot;
    for (uint32_t j = 0; j < cnt; j++) { held[sl] = base + (int64_t)(t0 + j); sl = sl + 1 == slots ? 0 : sl + 1; }
    while (k < n_out && m < t0 + cnt) {
      const size_t j = s.k0 + k;                 // the output on the period grid
      CHECK(m >= t0, "L %u M %u pos %u output %zu was due before this step", L, M, pos, k);
      CHECK(m + pos == j * M / L && ph == j * M % L && q == j % L, "L %u M %u pos %u output %zu: m %zu phase %u place %u", L, M, pos, k, m, ph, q);
      uint32_t si = wslot + (uint32_t)(m - t0);
      si = si >= slots ? si - slots : si;
      const uint32_t n_prod = k_full + (ph < rem ? 1u : 0u);
      for (uint32_t i = 0; i < n_prod; i++) {
        CHECK(held[si] == base + (int64_t)m - (int64_t)i, "L %u M %u taps %u pos %u output %zu product %u reads sample %lld", L, M, taps, pos, k, i, (long long)held[si]);
        si = si == 0 ? slots - 1 : si - 1;
      }
      k++;
      q = q + 1 == L ? 0 : q + 1;
      ph += M;
      while (ph >= L) { ph -= L; m++; }
    }
    wslot = sl;
  }
  CHECK(k == n_out, "L %u M %u taps %u pos %u: %zu outputs of %zu", L, M, taps, pos, k, n_out);
  const uint32_t hbase = (uint32_t)(n_high % slots);
  for (int64_t h = 0; h < H; h++) {
    uint32_t si = hbase + (uint32_t)h;
    si = si >= slots ? si - slots : si;
    CHECK(held[si] == base + (int64_t)n_high - H + h, "L %u M %u taps %u pos %u n_out %zu history %lld holds sample %lld", L, M, taps, pos, n_out, (long long)h, (long long)held[si]);
    ring_hist[(size_t)h] = held[si];
  }
  return n_high;
}

int main() {
  const uint32_t ratios[][2] = {{147, 160}, {160, 147}, {3, 2}, {2, 3}, {1, 6}, {6, 1}, {1, 1}, {255, 256}};
  for (const auto &r : ratios) {
    const uint32_t L = r[0], M = r[1];
    for (uint32_t pos = 0; pos < M; pos++)
      for (size_t n_out : {(size_t)1, (size_t)2, (size_t)L - 1, (size_t)L, (size_t)L + 1, (size_t)128, (size_t)129})
        if (n_out) check_start(L, M, pos, n_out);
    // a stream cut into calls of these counts, each from where the one before left the position and the history
    for (uint32_t taps : {1u, 2u, 7u, 31u, 97u, 2561u}) {
      const RatePlan P = processor_ratecvt_plan(L, taps, 1, true);
      const size_t H = resample_history(0, L, taps);
      std::vector<int64_t> hist(H ? H : 1);
      for (size_t h = 0; h < H; h++) hist[h] = (int64_t)h - (int64_t)H;
      int64_t base = 0;
      uint32_t pos = 0;
      size_t calls = 0;
      for (int round = 0; round < 12; round++) {
        for (size_t n_out : {(size_t)128, (size_t)1, (size_t)129, (size_t)147, (size_t)2, (size_t)1, (size_t)1, (size_t)L, (size_t)3}) {
          const size_t took = walk_call(L, M, taps, P.slots, pos, n_out, base, hist);
          if (!took) continue;                    // (L > M: a count this position cannot write)
          base += (int64_t)took;
          pos = ratecvt_next_position(M, pos, took);
          calls++;
        }
      }
      CHECK(calls >= 12, "L %u M %u taps %u: %zu calls", L, M, taps, calls);   // (M = 1: whole periods only, one call a round)
    }
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
