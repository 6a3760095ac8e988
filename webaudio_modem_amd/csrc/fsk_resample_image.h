// fsk_resample_image.h -- the image format of a resampler's snapshot (include/fskhip_next.h: "FSKR"), and the one definition of what
// makes an image valid: fskhip_resampler_snapshot_info_get, fskhip_resampler_restore (fsk_resample_remap_api.hip) and a stand-alone
// check program (tests/cpp/resample_image_check.cpp) all walk an image with rs_image_open.  Host-only: no HIP, plain C++ (which is
// why the frame's checks -- fsk_stage.h's image_open_front / _back, which need HIP and the library's error string -- are spelled
// here again, in their order, as fsk_xmodem_image.h does).  The caller's bytes need no alignment: every word is read with memcpy.
// Not part of the ABI.
//
//   RsImageHeader (48 bytes) | n_taps doubles, as given to create | n_records rows of `history` floats, packed | zeros to 16 bytes
//
// A history is plain floats and the taps are what create took, so nothing in an image depends on the build that wrote it: the
// format number is all a reader needs.  Any float is a valid history word (NaN payloads and signed zeros are carried bit for bit).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fsk_resample_plan.h"
#include "fsk_snapsum.h"

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
static_assert(sizeof(RsImageHeader) == 48, "RsImageHeader has padding");

inline uint64_t rs_round16(uint64_t n) { return (n + 15u) & ~(uint64_t)15u; }
inline uint64_t rs_live_bytes(uint32_t n_records, uint32_t n_taps, uint32_t history) {
  return sizeof(RsImageHeader) + (uint64_t)8u * n_taps + (uint64_t)4u * n_records * history;
}
inline uint64_t rs_image_bytes(uint32_t n_records, uint32_t n_taps, uint32_t history) { return rs_round16(rs_live_bytes(n_records, n_taps, history)); }

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

inline int rs_image_flaw(char *msg, size_t msg_cap, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
inline int rs_image_flaw(char *msg, size_t msg_cap, const char *fmt, ...) {
  if (msg && msg_cap) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, msg_cap, fmt, ap);
    va_end(ap);
  }
  return -1;
}

// 0 and *im filled in, or -1 and the flaw named in msg.  Order: null, a size below a header's, magic, format, header_bytes,
// direction, factor, n_taps, precision (create's limits), history against the design, record_bytes, the size against the layout,
// the checksum, the padding.
inline int rs_image_open(const void *buf, size_t size, RsImage *im, char *msg, size_t msg_cap) {
  RsImageHeader &h = im->h;
  if (!buf) return rs_image_flaw(msg, msg_cap, "null snapshot");
  if (size < sizeof(h)) return rs_image_flaw(msg, msg_cap, "%zu bytes are fewer than a resampler snapshot header's %zu", size, sizeof(h));
  std::memcpy(&h, buf, sizeof(h));
  if (h.magic != kRsMagic) return rs_image_flaw(msg, msg_cap, "not a resampler snapshot (magic 0x%08x, expected 0x%08x)", h.magic, kRsMagic);
  if (h.format != kRsFormat) return rs_image_flaw(msg, msg_cap, "resampler snapshot format %u, this library reads format %u", h.format, kRsFormat);
  if (h.header_bytes != sizeof(h)) return rs_image_flaw(msg, msg_cap, "header_bytes %u, expected %zu", h.header_bytes, sizeof(h));
  if (h.direction > 1u) return rs_image_flaw(msg, msg_cap, "direction %u is neither 0 (up) nor 1 (down)", h.direction);
  if (h.factor < 1u || h.factor > kResampleMaxFactor) return rs_image_flaw(msg, msg_cap, "factor %u outside 1..%u", h.factor, kResampleMaxFactor);
  if (h.n_taps < 1u || h.n_taps > kResampleMaxTaps) return rs_image_flaw(msg, msg_cap, "n_taps %u outside 1..%u", h.n_taps, kResampleMaxTaps);
  if (h.precision > 1u) return rs_image_flaw(msg, msg_cap, "precision %u is neither 0 (fp32) nor 1 (fp64)", h.precision);
  const uint32_t hist = resample_history((int)h.direction, h.factor, h.n_taps);
  if (h.history != hist)
    return rs_image_flaw(msg, msg_cap, "history %u, %u taps at factor %u %s keep %u", h.history, h.n_taps, h.factor, h.direction ? "down" : "up", hist);
  if (h.record_bytes != 4u * hist) return rs_image_flaw(msg, msg_cap, "record_bytes %u, a row of %u floats has %u", h.record_bytes, hist, 4u * hist);
  if (size != rs_image_bytes(h.n_records, h.n_taps, hist))
    return rs_image_flaw(msg, msg_cap, "%zu bytes do not match the layout (%zu + 8 x n_taps %u + n_records %u x record_bytes %u, rounded up to 16)", size,
                         sizeof(h), h.n_taps, h.n_records, h.record_bytes);
  const unsigned char *c = (const unsigned char *)buf;
  {
    RsImageHeader z = h;
    z.checksum = 0;
    SnapSum s;
    snap_sum(s, &z, sizeof(z));
    snap_sum(s, c + sizeof(h), size - sizeof(h));
    const uint64_t sum = snap_sum_value(s);
    if (sum != h.checksum)
      return rs_image_flaw(msg, msg_cap, "checksum %016llx, the bytes sum to %016llx (a damaged snapshot)", (unsigned long long)h.checksum, (unsigned long long)sum);
  }
  im->taps = c + sizeof(h);
  im->rows = im->taps + (size_t)8u * h.n_taps;
  const uint64_t live = rs_live_bytes(h.n_records, h.n_taps, hist);
  for (uint64_t i = live; i < size; i++)
    if (c[i] != 0) return rs_image_flaw(msg, msg_cap, "padding byte %llu behind the rows is 0x%02x, not zero", (unsigned long long)(i - live), c[i]);
  return 0;
}

}  // namespace fsk
