// fsk_ratecvt_image.h -- the image format of a rate converter's snapshot (include/fskhip_next.h: "FSKC"), and the one definition of
// what makes an image valid: fskhip_ratecvt_snapshot_info_get, fskhip_ratecvt_restore (fsk_ratecvt_remap_api.hip) and a stand-alone
// check program (tests/cpp/ratecvt_image_check.cpp) all walk an image with rc_image_open, on fsk_image.h's frame.  Host-only: no
// HIP, plain C++.  The caller's bytes need no alignment: every word is read with memcpy.  Not part of the ABI.
//
//   RcImageHeader (64 bytes) | n_taps doubles, as given to create | n_records rows of `history` floats, packed | zeros to 16 bytes
//
// A history is plain floats, the taps are what create took and the position is a count of inputs, so nothing in an image depends on
// the build that wrote it: the format number is all a reader needs.  Any float is a valid history word (NaN payloads and signed
// zeros are carried bit for bit).  The device's tap order and the per-period table are create's to make, never an image's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fsk_image.h"
#include "fsk_ratecvt_plan.h"
#include "fsk_resample_image.h"

namespace fsk {

constexpr uint32_t kRcMagic = 0x434B5346u;   // "FSKC"
constexpr uint32_t kRcFormat = 1;

struct RcImageHeader {
  uint32_t magic, format;
  uint32_t header_bytes, record_bytes;   // record_bytes = 4 * history
  uint32_t n_records, direction;         // direction: 0 capture, 1 playback (FSKHIP_RATECVT_*)
  uint32_t up, down;                     // coprime, each 1..kRatecvtMaxFactor
  uint32_t n_taps, precision;            // precision: 0 fp32, 1 fp64 (FSKHIP_PRECISION_*)
  uint32_t history, position;            // history = resample_history(0, up, n_taps); position < down: the one word of all streams
  uint32_t reserved[2];                  // zero
  uint64_t checksum;                     // snap_sum over the whole image with this field 0
};
static_assert(sizeof(RcImageHeader) == 64 && offsetof(RcImageHeader, magic) == 0 && offsetof(RcImageHeader, format) == 4 && offsetof(RcImageHeader, header_bytes) == 8 &&
              offsetof(RcImageHeader, n_records) == 16 && offsetof(RcImageHeader, up) == 24 && offsetof(RcImageHeader, history) == 40 &&
              offsetof(RcImageHeader, reserved) == 48 && offsetof(RcImageHeader, checksum) == 56, "RcImageHeader is format 1's");

inline uint64_t rc_live_bytes(uint32_t n_records, uint32_t n_taps, uint32_t history) {
  return sizeof(RcImageHeader) + (uint64_t)8u * n_taps + (uint64_t)4u * n_records * history;
}
inline uint64_t rc_image_bytes(uint32_t n_records, uint32_t n_taps, uint32_t history) { return image_round16(rc_live_bytes(n_records, n_taps, history)); }

// a validated image: the header (copied), the taps and the rows in the caller's bytes
struct RcImage {
  RcImageHeader h;
  const unsigned char *taps, *rows;
  double tap(uint32_t i) const {
    double v;
    std::memcpy(&v, taps + (size_t)8u * i, 8);
    return v;
  }
};

// 0 and *im filled in, or -1 and the flaw named in msg.  Order: null, a size below a header's, magic (a resampler's image is
// named), format, header_bytes, the reserved words, direction, up, down, lowest terms, n_taps, precision (create's limits),
// history against the design, position against down, record_bytes, the size against the layout, the checksum, the padding.
inline int rc_image_open(const void *buf, size_t size, RcImage *im, char *msg, size_t msg_cap) {
  RcImageHeader &h = im->h;
  if (const int rc = image_open_front("a rate converter snapshot", buf, size, kRcMagic, kRcFormat, &h, msg, msg_cap)) {
    if (buf && size >= sizeof(h) && h.magic == kRsMagic)   // (the likeliest stranger names itself)
      return image_flaw(msg, msg_cap, "not a rate converter snapshot (magic 0x%08x is a resampler snapshot's, expected 0x%08x)", h.magic, kRcMagic);
    return rc;
  }
  if (h.reserved[0] != 0u || h.reserved[1] != 0u) return image_flaw(msg, msg_cap, "reserved words 0x%08x 0x%08x are not zero", h.reserved[0], h.reserved[1]);
  if (h.direction > 1u) return image_flaw(msg, msg_cap, "direction %u is neither 0 (capture) nor 1 (playback)", h.direction);
  if (h.up < 1u || h.up > kRatecvtMaxFactor) return image_flaw(msg, msg_cap, "up %u outside 1..%u", h.up, kRatecvtMaxFactor);
  if (h.down < 1u || h.down > kRatecvtMaxFactor) return image_flaw(msg, msg_cap, "down %u outside 1..%u", h.down, kRatecvtMaxFactor);
  if (ratecvt_gcd(h.up, h.down) != 1u) return image_flaw(msg, msg_cap, "%u / %u is not in lowest terms", h.up, h.down);
  if (h.n_taps < 1u || h.n_taps > kResampleMaxTaps) return image_flaw(msg, msg_cap, "n_taps %u outside 1..%u", h.n_taps, kResampleMaxTaps);
  if (h.precision > 1u) return image_flaw(msg, msg_cap, "precision %u is neither 0 (fp32) nor 1 (fp64)", h.precision);
  const uint32_t hist = resample_history(0, h.up, h.n_taps);
  if (h.history != hist) return image_flaw(msg, msg_cap, "history %u, %u taps at an up factor of %u keep %u", h.history, h.n_taps, h.up, hist);
  if (h.position >= h.down) return image_flaw(msg, msg_cap, "position %u is not below the down factor %u", h.position, h.down);
  if (h.record_bytes != 4u * hist) return image_flaw(msg, msg_cap, "record_bytes %u, a row of %u floats has %u", h.record_bytes, hist, 4u * hist);
  if (size != rc_image_bytes(h.n_records, h.n_taps, hist))
    return image_flaw(msg, msg_cap, "%zu bytes do not match the layout (%zu + 8 x n_taps %u + n_records %u x record_bytes %u, rounded up to 16)", size,
                      sizeof(h), h.n_taps, h.n_records, h.record_bytes);
  if (const int rc = image_check_sum(buf, size, h, msg, msg_cap)) return rc;
  im->taps = (const unsigned char *)buf + sizeof(h);
  im->rows = im->taps + (size_t)8u * h.n_taps;
  return image_check_padding("the rows", (const unsigned char *)buf, rc_live_bytes(h.n_records, h.n_taps, hist), size, msg, msg_cap);
}

}  // namespace fsk
