// fsk_xmodem_image.h -- the image format of the resident XModem handles' snapshots (include/fskhip_next.h: "FSKX"), and the one
// definition of what makes an image valid: fskhip_xmodem_snapshot_info_get, the three restores (fsk_xmodem_remap_api.hip) and a
// stand-alone check program (tests/cpp/xmodem_snapshot_check.cpp) all walk an image with xm_image_open, on fsk_image.h's frame.
// Host-only: no HIP, plain C++.  The caller's bytes need no alignment: every word is read with memcpy.  Not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fsk_image.h"

namespace fsk {

constexpr uint32_t kXmMagic = 0x584B5346u;   // "FSKX"
constexpr uint32_t kXmFormat = 1;
enum : uint32_t { kXmKindRx = 1, kXmKindTx = 2, kXmKindRecv = 3 };

struct XmImageHeader {
  uint32_t magic, format;
  uint32_t header_bytes, kind;
  uint32_t n_records, record_words;
  uint32_t param0, param1;   // rx: 0 / 0; tx: max_payload_size / max_retries; recv: file_capacity / max_retries
  uint64_t checksum;         // snap_sum over the whole image with this field 0
  uint64_t file_bytes;       // the records' file lengths, summed
};
static_assert(sizeof(XmImageHeader) == 48 && offsetof(XmImageHeader, magic) == 0 && offsetof(XmImageHeader, format) == 4 && offsetof(XmImageHeader, header_bytes) == 8 &&
              offsetof(XmImageHeader, n_records) == 16 && offsetof(XmImageHeader, checksum) == 32, "XmImageHeader is format 1's");

inline uint32_t xm_record_words(uint32_t kind) { return kind == kXmKindRx ? 4u : (kind == kXmKindTx || kind == kXmKindRecv) ? 8u : 0u; }
inline const char *xm_kind_name(uint32_t kind) { return kind == kXmKindRx ? "rx" : kind == kXmKindTx ? "tx" : kind == kXmKindRecv ? "recv" : "?"; }
// the position of a record's file length among its words (rx records have none)
inline int xm_file_len_word(uint32_t kind) { return kind == kXmKindTx ? 6 : kind == kXmKindRecv ? 3 : -1; }
inline size_t xm_image_bytes(uint32_t n_records, uint32_t record_words, uint64_t file_bytes) {
  return sizeof(XmImageHeader) + (size_t)4u * n_records * record_words + (size_t)image_round16(file_bytes);
}
// XModemTransport's fragment count (xmodem.ts:103-107): an empty file is one empty fragment
inline uint64_t xm_fragments(uint64_t len, uint32_t max_payload) { return len == 0u ? 1u : (len + max_payload - 1u) / max_payload; }

// a validated image: the header (copied), the word table and the file area in the caller's bytes
struct XmImage {
  XmImageHeader h;
  const unsigned char *table, *files;
  uint32_t word(uint32_t record, uint32_t k) const {
    uint32_t v;
    std::memcpy(&v, table + ((size_t)record * h.record_words + k) * 4u, 4);
    return v;
  }
  uint32_t file_len(uint32_t record) const { return xm_file_len_word(h.kind) < 0 ? 0u : word(record, (uint32_t)xm_file_len_word(h.kind)); }
};

// 0 and *im filled in, or -1 and the flaw named in msg.  Order: null, a size below a header's, magic, format, header_bytes, kind,
// record_words, the size against the layout, the checksum, the file lengths against file_bytes, padding and reserved words, then
// record by record.
inline int xm_image_open(const void *buf, size_t size, XmImage *im, char *msg, size_t msg_cap) {
  XmImageHeader &h = im->h;
  if (const int rc = image_open_front("an XModem snapshot", buf, size, kXmMagic, kXmFormat, &h, msg, msg_cap)) return rc;
  if (xm_record_words(h.kind) == 0u) return image_flaw(msg, msg_cap, "kind %u is none of 1 (rx), 2 (tx), 3 (recv)", h.kind);
  if (h.record_words != xm_record_words(h.kind))
    return image_flaw(msg, msg_cap, "record_words %u, a %s record has %u", h.record_words, xm_kind_name(h.kind), xm_record_words(h.kind));
  const size_t table_bytes = (size_t)4u * h.n_records * h.record_words;
  if (h.file_bytes > size || size != xm_image_bytes(h.n_records, h.record_words, h.file_bytes))
    return image_flaw(msg, msg_cap, "%zu bytes do not match the layout (%zu + 4 x n_records %u x record_words %u + file_bytes %llu rounded up to 16)", size,
                      sizeof(h), h.n_records, h.record_words, (unsigned long long)h.file_bytes);
  if (const int rc = image_check_sum(buf, size, h, msg, msg_cap)) return rc;
  im->table = (const unsigned char *)buf + sizeof(h);
  im->files = im->table + table_bytes;
  uint64_t total = 0;
  for (uint32_t r = 0; r < h.n_records; r++) total += im->file_len(r);
  if (total != h.file_bytes)
    return image_flaw(msg, msg_cap, "the records' file_len sum to %llu, file_bytes is %llu", (unsigned long long)total, (unsigned long long)h.file_bytes);
  if (const int rc = image_check_padding("the files", im->files, h.file_bytes, image_round16(h.file_bytes), msg, msg_cap)) return rc;
  if (h.kind == kXmKindRx && (h.param0 != 0u || h.param1 != 0u)) return image_flaw(msg, msg_cap, "reserved header words (param0 %u, param1 %u) of an rx image are not zero", h.param0, h.param1);
  if (h.kind == kXmKindTx && (h.param0 < 1u || h.param0 > 255u)) return image_flaw(msg, msg_cap, "param0 (max_payload_size) %u is not in 1..255", h.param0);
  for (uint32_t r = 0; r < h.n_records; r++) {
    uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < h.record_words; k++) w[k] = im->word(r, k);
    if (h.kind == kXmKindRx) {
      if (w[0] < 1u || w[0] > 255u) return image_flaw(msg, msg_cap, "record %u: expected %u is not a sequence number (1-255)", r, w[0]);
      if (w[3] != 0u) return image_flaw(msg, msg_cap, "record %u: reserved word 3 is %u, not zero", r, w[3]);
    } else if (h.kind == kXmKindTx) {
      if (w[0] > 3u) return image_flaw(msg, msg_cap, "record %u: state %u is not a state (0-3)", r, w[0]);
      if (w[1] < 1u || w[1] > 255u) return image_flaw(msg, msg_cap, "record %u: sequence %u is not a sequence number (1-255)", r, w[1]);
      if (w[7] > 1u) return image_flaw(msg, msg_cap, "record %u: has_file %u is neither 0 nor 1", r, w[7]);
      if (w[7] == 0u && w[6] != 0u) return image_flaw(msg, msg_cap, "record %u: file_len %u without a file (has_file 0)", r, w[6]);
      if (w[0] == 1u || w[0] == 2u) {   // WAIT_NAK, WAIT_ACK: a fragment is about to go out
        if (w[7] == 0u) return image_flaw(msg, msg_cap, "record %u: state %u waits to send a fragment, but no file is held (has_file 0)", r, w[0]);
        if (w[2] >= xm_fragments(w[6], h.param0))
          return image_flaw(msg, msg_cap, "record %u: fragment_index %u of %llu fragments (file_len %u, max_payload_size %u)", r, w[2],
                            (unsigned long long)xm_fragments(w[6], h.param0), w[6], h.param0);
      }
    } else {
      if (w[0] > 3u) return image_flaw(msg, msg_cap, "record %u: state %u is not a state (0-3)", r, w[0]);
      if (w[1] < 1u || w[1] > 255u) return image_flaw(msg, msg_cap, "record %u: expected %u is not a sequence number (1-255)", r, w[1]);
      if (w[3] > h.param0) return image_flaw(msg, msg_cap, "record %u: file_len %u exceeds file_capacity %u", r, w[3], h.param0);
      if (w[7] != 0u) return image_flaw(msg, msg_cap, "record %u: reserved word 7 is %u, not zero", r, w[7]);
    }
  }
  return 0;
}

}  // namespace fsk
