// fsk_xmodem_timer_image.h -- the image format of the XModem wait timers' snapshots (include/fskhip_next.h: "FSKW"), and the one
// definition of what makes an image valid: fskhip_xmodem_timer_snapshot_info_get, fskhip_xmodem_timer_restore
// (fsk_xmodem_timer_api.hip) and a stand-alone check program (tests/cpp/xmodem_timer_image_check.cpp) all walk an image with
// xw_image_open, on fsk_image.h's frame.  Host-only: no HIP, plain C++.  The caller's bytes need no alignment: every word is read
// with memcpy.  Not part of the ABI.
//
//   XwImageHeader (48 bytes, the XModem image's field offsets) | n_records x (waited, mark) | zeros to 16 bytes
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fsk_image.h"
#include "fsk_xmodem_timer.h"

namespace fsk {

constexpr uint32_t kXwMagic = 0x574B5346u;    // "FSKW"
constexpr uint32_t kXwXmMagic = 0x584B5346u;  // "FSKX": a handle's own image (fsk_xmodem_image.h), the likeliest stranger
constexpr uint32_t kXwFormat = 1;
constexpr uint32_t kXwRecordWords = 2;
enum : uint32_t { kXwKindTx = 2, kXwKindRecv = 3 };   // fsk_xmodem_image.h's numbers

struct XwImageHeader {
  uint32_t magic, format;
  uint32_t header_bytes, kind;
  uint32_t n_records, record_words;
  uint32_t timeout_samples, reserved0;   // the writer's timeout, for a reader that wants it; zero
  uint64_t checksum;                     // snap_sum over the whole image with this field 0
  uint64_t reserved1;                    // zero
};
static_assert(sizeof(XwImageHeader) == 48 && offsetof(XwImageHeader, magic) == 0 && offsetof(XwImageHeader, format) == 4 && offsetof(XwImageHeader, header_bytes) == 8 &&
              offsetof(XwImageHeader, n_records) == 16 && offsetof(XwImageHeader, timeout_samples) == 24 && offsetof(XwImageHeader, checksum) == 32,
              "XwImageHeader is format 1's");

inline const char *xw_kind_name(uint32_t kind) { return kind == kXwKindTx ? "tx" : kind == kXwKindRecv ? "recv" : "?"; }
inline uint64_t xw_live_bytes(uint32_t n_records) { return sizeof(XwImageHeader) + (uint64_t)4u * kXwRecordWords * n_records; }
inline uint64_t xw_image_bytes(uint32_t n_records) { return image_round16(xw_live_bytes(n_records)); }

// a validated image: the header (copied) and the records in the caller's bytes
struct XwImage {
  XwImageHeader h;
  const unsigned char *table;
  xw::Words record(uint32_t r) const {
    xw::Words T;
    std::memcpy(&T.waited, table + (size_t)8u * r, 4);
    std::memcpy(&T.mark, table + (size_t)8u * r + 4u, 4);
    return T;
  }
};

// 0 and *im filled in, or -1 and the flaw named in msg.  Order: null, a size below a header's, magic (a handle's image is named),
// format, header_bytes, kind, record_words, timeout_samples, the reserved fields, the size against the layout, the checksum, the
// padding, then record by record what fskhip_xmodem_timer_state_set asks of a mark.
inline int xw_image_open(const void *buf, size_t size, XwImage *im, char *msg, size_t msg_cap) {
  XwImageHeader &h = im->h;
  if (const int rc = image_open_front("an XModem timer snapshot", buf, size, kXwMagic, kXwFormat, &h, msg, msg_cap)) {
    if (buf && size >= sizeof(h) && h.magic == kXwXmMagic)
      return image_flaw(msg, msg_cap, "not an XModem timer snapshot (magic 0x%08x is an XModem handle's snapshot's, expected 0x%08x)", h.magic, kXwMagic);
    return rc;
  }
  if (h.kind != kXwKindTx && h.kind != kXwKindRecv) return image_flaw(msg, msg_cap, "kind %u is neither 2 (tx) nor 3 (recv)", h.kind);
  if (h.record_words != kXwRecordWords) return image_flaw(msg, msg_cap, "record_words %u, a timer record has %u", h.record_words, kXwRecordWords);
  if (h.timeout_samples == 0u) return image_flaw(msg, msg_cap, "timeout_samples is 0");
  if (h.reserved0 != 0u || h.reserved1 != 0u)
    return image_flaw(msg, msg_cap, "reserved header fields 0x%08x 0x%016llx are not zero", h.reserved0, (unsigned long long)h.reserved1);
  if (size != xw_image_bytes(h.n_records))
    return image_flaw(msg, msg_cap, "%zu bytes do not match the layout (%zu + 8 x n_records %u, rounded up to 16)", size, sizeof(h), h.n_records);
  if (const int rc = image_check_sum(buf, size, h, msg, msg_cap)) return rc;
  im->table = (const unsigned char *)buf + sizeof(h);
  if (const int rc = image_check_padding("the records", (const unsigned char *)buf, xw_live_bytes(h.n_records), size, msg, msg_cap)) return rc;
  for (uint32_t r = 0; r < h.n_records; r++) {
    const uint32_t mark = im->record(r).mark;
    if (!xw::valid_mark(mark)) return image_flaw(msg, msg_cap, "record %u: mark %u is not a mark (stage 0-2, plus 4 for was-pending)", r, mark);
    if (h.kind == kXwKindTx && (mark & xw::kStageMask)) return image_flaw(msg, msg_cap, "record %u: mark %u has a stage, a sender's timer has none", r, mark);
  }
  return 0;
}

}  // namespace fsk
