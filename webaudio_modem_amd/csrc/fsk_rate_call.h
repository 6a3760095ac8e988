// fsk_rate_call.h -- what a process call of the two rate converters (fsk_resample.hip, fsk_ratecvt.hip) is refused for behind the
// null handle, in plain C++ so that it also compiles without HIP (tests/cpp/rate_call_check.cpp).  Not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fskhip.h"

namespace fsk {

// One _device or _host call as plain values.  `narrow` is the side in the capture format, `wide` the float32 rows; the counts
// are elements per stream (of a call that passes the last check), the pitches are in elements, the pointers are numbers.
struct RateCall {
  size_t n_in, n_narrow, n_wide;
  uint32_t n_streams;
  uintptr_t narrow, wide, lens;
  size_t narrow_pitch, wide_pitch;
  size_t esz;          // bytes of the format's element (sample_bytes), 0 where the format is none
  int layout;
  size_t multiple;     // n_in must be a multiple of it (1: any)
  bool direction_ok;   // the handle was created for the call's direction
};

enum class RateRefusal { none, format, layout, null_buffer, float_pitch, sample_pitch, frame_pitch, alignment, direction, multiple };

// The first refusal in the header's order: format and layout; then, for a call that has samples, null buffers, the pitches and
// the alignments (device pointers are held to their element's alignment, host pointers too); the handle's direction; an n_in
// that is no multiple.
inline RateRefusal rate_call_check(const RateCall &c) {
  if (!c.esz) return RateRefusal::format;
  if (c.layout != FSKHIP_LAYOUT_STREAM_MAJOR && c.layout != FSKHIP_LAYOUT_SAMPLE_MAJOR) return RateRefusal::layout;
  if (c.n_in > 0) {
    if (!c.narrow || !c.wide) return RateRefusal::null_buffer;
    if (c.wide_pitch < c.n_wide) return RateRefusal::float_pitch;
    if (c.layout == FSKHIP_LAYOUT_STREAM_MAJOR && c.narrow_pitch < c.n_narrow) return RateRefusal::sample_pitch;
    if (c.layout == FSKHIP_LAYOUT_SAMPLE_MAJOR && c.narrow_pitch < c.n_streams) return RateRefusal::frame_pitch;
    if ((c.wide & 3u) != 0 || (c.lens & 3u) != 0 || (c.narrow & (c.esz - 1u)) != 0) return RateRefusal::alignment;
  }
  if (!c.direction_ok) return RateRefusal::direction;
  if (c.n_in % c.multiple != 0) return RateRefusal::multiple;
  return RateRefusal::none;
}

}  // namespace fsk
