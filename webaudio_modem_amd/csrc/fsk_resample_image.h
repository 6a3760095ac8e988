// fsk_resample_image.h -- the image format of a resampler's snapshot (include/fskhip_next.h: "FSKR"), and the one definition of what
// makes an image valid: fskhip_resampler_snapshot_info_get, fskhip_resampler_restore (fsk_resample_remap_api.hip) and a stand-alone
// check program (tests/cpp/resample_image_check.cpp) all walk an image with rs_image_open, on fsk_image.h's frame.  Host-only: no
// HIP, plain C++.  The caller's bytes need no alignment: every word is read with memcpy.  Not part of the ABI.
//
//   RsImageHeader (48 bytes) | n_taps doubles, as given to create | n_records rows of `history` floats, packed | zeros to 16 bytes
//
// A history is plain floats and the taps are what create took, so nothing in an image depends on the build that wrote it: the
// format number is all a reader needs.  Any float is a valid history word (NaN payloads and signed zeros are carried bit for bit).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fsk_image.h"
#include "fsk_resample_plan.h"

namespace fsk {

constexpr uint32_t kRsMagic = 0x524B5346u;   // "FSKR"
constexpr uint32_t kRsFormat = 1;

struct RsImageHeader {
  uint32_t magic, format;
  uint32_t header_bytes, record_bytes;   // record_bytes = 4 * history
  uint32_t n_records, direction;         // direction: 0 up, 1 down (FSKHIP_RESAMPLE_*)
  uint32_t factor, n_taps;
  uint32_t precision, history;           // precision: 0 fp32, 1 fp64 (FSKHIP_PRECISION_*); history = resample_history(direction, factor, n_taps)
  uint64_t checksum;                     // snap_sum over the whole image with this field 0
};
static_assert(sizeof(RsImageHeader) == 48 && offsetof(RsImageHeader, magic) == 0 && offsetof(RsImageHeader, format) == 4 && offsetof(RsImageHeader, header_bytes) == 8 &&
              offsetof(RsImageHeader, n_records) == 16 && offsetof(RsImageHeader, checksum) == 40, "RsImageHeader is format 1's");

inline uint64_t rs_live_bytes(uint32_t n_records, uint32_t n_taps, uint32_t history) {
  return sizeof(RsImageHeader) + (uint64_t)8u * n_taps + (uint64_t)4u * n_records * history;
}
inline uint64_t rs_image_bytes(uint32_t n_records, uint32_t n_taps, uint32_t history) { return image_round16(rs_live_bytes(n_records, n_taps, history)); }

// a validated image: the header (copied), the taps and the rows in the caller's bytes
struct RsImage {
  RsImageHeader h;
  const unsigned char *taps, *rows;
  double tap(uint32_t i) const {
    double v;
    std::memcpy(&v, taps + (size_t)8u * i, 8);
    return v;
  }
};

// 0 and *im filled in, or -1 and the flaw named in msg.  Order: null, a size below a header's, magic, format, header_bytes,
// direction, factor, n_taps, precision (create's limits), history against the design, record_bytes, the size against the layout,
// the checksum, the padding.
inline int rs_image_open(const void *buf, size_t size, RsImage *im, char *msg, size_t msg_cap) {
  RsImageHeader &h = im->h;
  if (const int rc = image_open_front("a resampler snapshot", buf, size, kRsMagic, kRsFormat, &h, msg, msg_cap)) return rc;
  if (h.direction > 1u) return image_flaw(msg, msg_cap, "direction %u is neither 0 (up) nor 1 (down)", h.direction);
  if (h.factor < 1u || h.factor > kResampleMaxFactor) return image_flaw(msg, msg_cap, "factor %u outside 1..%u", h.factor, kResampleMaxFactor);
  if (h.n_taps < 1u || h.n_taps > kResampleMaxTaps) return image_flaw(msg, msg_cap, "n_taps %u outside 1..%u", h.n_taps, kResampleMaxTaps);
  if (h.precision > 1u) return image_flaw(msg, msg_cap, "precision %u is neither 0 (fp32) nor 1 (fp64)", h.precision);
  const uint32_t hist = resample_history((int)h.direction, h.factor, h.n_taps);
  if (h.history != hist)
    return image_flaw(msg, msg_cap, "history %u, %u taps at factor %u %s keep %u", h.history, h.n_taps, h.factor, h.direction ? "down" : "up", hist);
  if (h.record_bytes != 4u * hist) return image_flaw(msg, msg_cap, "record_bytes %u, a row of %u floats has %u", h.record_bytes, hist, 4u * hist);
  if (size != rs_image_bytes(h.n_records, h.n_taps, hist))
    return image_flaw(msg, msg_cap, "%zu bytes do not match the layout (%zu + 8 x n_taps %u + n_records %u x record_bytes %u, rounded up to 16)", size,
                      sizeof(h), h.n_taps, h.n_records, h.record_bytes);
  if (const int rc = image_check_sum(buf, size, h, msg, msg_cap)) return rc;
  im->taps = (const unsigned char *)buf + sizeof(h);
  im->rows = im->taps + (size_t)8u * h.n_taps;
  return image_check_padding("the rows", (const unsigned char *)buf, rs_live_bytes(h.n_records, h.n_taps, hist), size, msg, msg_cap);
}

}  // namespace fsk
