// rate_call_check.cpp -- what a process call of the two rate converters is refused for behind the null handle
// (webaudio_modem_amd/csrc/fsk_rate_call.h) from a program of its own, for a sanitizer run without a GPU.
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I webaudio_modem_amd/csrc
//     tests/cpp/rate_call_check.cpp -o rate_call_check && ./rate_call_check
// For the resampler (up, down; factors 1 and 6) and the rate converter (capture, playback; 160/147, 147/160, 3/2), with the counts
// and the multiple each unit hands over (fsk_resample.hip, fsk_ratecvt.hip: process), every element size and both layouts: a call
// with everything wrong is put right one step at a time, in the header's order, and each step must meet the next refusal -- so
// every refusal is met with all behind it wrong as well --; the null buffers and the misalignments one by one; the well-formed
// call last; and an empty call, which is held to its format, layout and direction alone.  Prints "ok" and exits 0, else the
// first failures.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "fsk_rate_call.h"
#include "fsk_ratecvt_plan.h"

using namespace fsk;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (failures++ < 20) { std::printf("line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                           \
  } while (0)

// a unit's direction: which side is read, what a call of n_in writes, what n_in must be a multiple of
struct Way { const char *name; bool narrow_in; uint32_t L, M; bool ratio; };
static size_t out_count(const Way &w, size_t n_in) { return w.ratio ? ratecvt_out_count(w.L, w.M, n_in) : resample_out_count(w.narrow_in ? 0 : 1, w.L, n_in); }
static size_t multiple(const Way &w) { return w.ratio ? w.M : w.narrow_in ? 1u : w.L; }

static void counts(RateCall &c, const Way &w, size_t n_in) {
  c.n_in = n_in;
  c.n_narrow = w.narrow_in ? n_in : out_count(w, n_in);
  c.n_wide = w.narrow_in ? out_count(w, n_in) : n_in;
}

static void walk(const Way &w, size_t esz, int layout) {
  const size_t m = multiple(w);
  const uint32_t S = 5;
  const uintptr_t base = 0x10000;   // (aligned to every element)
#define MEETS(what) CHECK(rate_call_check(c) == RateRefusal::what, "%s esz %zu layout %d: met %d", w.name, esz, layout, (int)rate_call_check(c))
  RateCall c{};
  counts(c, w, 2 * m + 1);          // no multiple where m > 1, and at least one element on either side
  c.n_streams = S; c.multiple = m;
  c.narrow = c.wide = 0; c.lens = base + 2; c.narrow_pitch = c.wide_pitch = 0;
  c.esz = 0; c.layout = 7; c.direction_ok = false;
  CHECK(c.n_narrow >= 1 && c.n_wide >= 1, "%s", w.name);
  MEETS(format);
  c.esz = esz;
  MEETS(layout);
  c.layout = -1;
  MEETS(layout);
  c.layout = layout;
  MEETS(null_buffer);
  c.narrow = base + 1; c.wide = 0;
  MEETS(null_buffer);
  c.narrow = 0; c.wide = base + 1;
  MEETS(null_buffer);
  c.narrow = base + 1;
  MEETS(float_pitch);
  c.wide_pitch = c.n_wide - 1;
  MEETS(float_pitch);
  c.wide_pitch = c.n_wide;
  if (layout == FSKHIP_LAYOUT_STREAM_MAJOR) {
    MEETS(sample_pitch);
    c.narrow_pitch = c.n_narrow - 1;
    MEETS(sample_pitch);
    c.narrow_pitch = c.n_narrow;     // (below the stream count where that is larger: stream-major does not look at it)
  } else {
    MEETS(frame_pitch);
    c.narrow_pitch = S - 1;          // (may be above n_narrow: frames do not look at it)
    MEETS(frame_pitch);
    c.narrow_pitch = S;
  }
  MEETS(alignment);                  // all three
  c.narrow = base; c.lens = 0;       // the float rows alone; no lens is aligned
  MEETS(alignment);
  c.wide = base + 2;
  MEETS(alignment);
  c.wide = base; c.lens = base + 2;  // the lens alone
  MEETS(alignment);
  c.lens = base + 4;
  for (uintptr_t off = 1; off < esz; off++) {   // the narrow side alone, by every offset within its element
    c.narrow = base + off;
    MEETS(alignment);
  }
  c.narrow = base + esz;             // aligned to its element and no further
  MEETS(direction);
  c.direction_ok = true;
  if (m > 1) {
    MEETS(multiple);
    counts(c, w, c.n_in - 2);
    MEETS(multiple);
  }
  counts(c, w, 2 * m);               // the pitches above still hold these
  MEETS(none);
  c.lens = 0;
  MEETS(none);
  c.wide_pitch = c.n_wide + 3; c.narrow_pitch += 3;
  MEETS(none);

  // an empty call: nothing of the buffers is looked at
  RateCall e{};
  e.n_streams = S; e.multiple = m; e.lens = base + 1; e.esz = 0; e.layout = 2; e.direction_ok = false;
  c = e;
  MEETS(format);
  c.esz = esz;
  MEETS(layout);
  c.layout = layout;
  MEETS(direction);
  c.direction_ok = true;
  MEETS(none);
#undef MEETS
}

int main() {
  const Way ways[] = {{"up 1", true, 1, 1, false},           {"up 6", true, 6, 1, false},           {"down 1", false, 1, 1, false},
                      {"down 6", false, 6, 1, false},        {"capture 160/147", true, 160, 147, true}, {"playback 147/160", false, 147, 160, true},
                      {"capture 147/160", true, 147, 160, true}, {"playback 160/147", false, 160, 147, true}, {"capture 3/2", true, 3, 2, true},
                      {"playback 3/2", false, 3, 2, true},   {"capture 1/1", true, 1, 1, true},     {"playback 1/1", false, 1, 1, true}};
  for (const Way &w : ways)
    for (const size_t esz : {(size_t)4, (size_t)2, (size_t)1})
      for (const int layout : {(int)FSKHIP_LAYOUT_STREAM_MAJOR, (int)FSKHIP_LAYOUT_SAMPLE_MAJOR}) walk(w, esz, layout);
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
