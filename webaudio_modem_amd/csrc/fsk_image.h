// fsk_image.h -- the frame every snapshot image of this library has, once for the five formats (fsk_snapshot_image.h,
// fsk_processor_image.h, fsk_xmodem_image.h, fsk_resample_image.h, fsk_ratecvt_image.h): a header `H` that names magic, format, header_bytes and checksum
// -- wherever the format puts them --, a body behind it, a checksum over both; a writer's header and seal, a reader's checks and
// their texts.  Host-only: no HIP and no error string of the library's, so that a format's validator compiles into a stand-alone
// check program (tests/cpp): a flaw is named in the caller's `msg` (fsk_host.h: open_image).  Not part of the ABI.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace fsk {

// Running position-dependent sum over little-endian 64-bit words (sizes here are multiples of 8): a = sum of words, b = sum of
// the running a.  Two adds per 8 bytes -- it runs at memory speed, which a byte-wise hash of a 66 MB image would not.
struct SnapSum { uint64_t a = 0, b = 0; };
inline void snap_sum(SnapSum &s, const void *p, size_t bytes) {
  const unsigned char *c = (const unsigned char *)p;
  uint64_t a = s.a, b = s.b;
  for (size_t i = 0; i + 8 <= bytes; i += 8) {
    uint64_t w;
    std::memcpy(&w, c + i, 8);
    a += w; b += a;
  }
  s.a = a; s.b = b;
}
inline uint64_t snap_sum_value(const SnapSum &s) { return s.a * 0x9E3779B97F4A7C15ull ^ s.b; }

// the flaw of an image, named in msg: -1
__attribute__((format(printf, 3, 4))) inline int image_flaw(char *msg, size_t msg_cap, const char *fmt, ...) {
  if (msg && msg_cap) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, msg_cap, fmt, ap);
    va_end(ap);
  }
  return -1;
}

inline uint64_t image_round16(uint64_t n) { return (n + 15u) & ~(uint64_t)15u; }

// the checksum of an image: over the header with its checksum field 0, then the body
template <class H>
uint64_t image_checksum(H h, const void *body, size_t bytes) {
  h.checksum = 0;
  SnapSum s;
  snap_sum(s, &h, sizeof(h));
  snap_sum(s, body, bytes);
  return snap_sum_value(s);
}

// a writer's header: zeroed (every byte of an image is defined), the frame's fields set; the format fills in the rest
template <class H>
H image_header(uint32_t magic, uint32_t format) {
  H h;
  std::memset(&h, 0, sizeof(h));
  h.magic = magic; h.format = format; h.header_bytes = sizeof(H);
  return h;
}

// a writer's last step: the body of an image of `size` bytes stands behind the header's place in buf
template <class H>
void image_seal(H h, void *buf, size_t size) {
  h.checksum = image_checksum(h, (const unsigned char *)buf + sizeof(H), size - sizeof(H));
  std::memcpy(buf, &h, sizeof(H));
}

// The front of opening an image: null, shorter than a header, magic, format, header_bytes.  `a_noun` is what the messages call
// the image, with its article ("an XModem snapshot").  The header is copied to *h.  `stamp`: a format's check that goes between
// format and header_bytes (which build wrote the image), returning 0 or its image_flaw.
template <class H, class Stamp = int (*)()>
int image_open_front(const char *a_noun, const void *buf, size_t size, uint32_t magic, uint32_t format, H *h, char *msg, size_t msg_cap,
                     Stamp stamp = [] { return 0; }) {
  if (!buf) return image_flaw(msg, msg_cap, "null snapshot");
  if (size < sizeof(H)) return image_flaw(msg, msg_cap, "%zu bytes are fewer than %s header's %zu", size, a_noun, sizeof(H));
  std::memcpy(h, buf, sizeof(H));
  if (h->magic != magic) return image_flaw(msg, msg_cap, "not %s (magic 0x%08x, expected 0x%08x)", a_noun, h->magic, magic);
  if (h->format != format) return image_flaw(msg, msg_cap, "%s format %u, this library reads format %u", std::strchr(a_noun, ' ') + 1, h->format, format);
  if (const int rc = stamp()) return rc;
  if (h->header_bytes != sizeof(H)) return image_flaw(msg, msg_cap, "header_bytes %u, expected %zu", h->header_bytes, sizeof(H));
  return 0;
}

// the bytes behind the header sum to the header's checksum
template <class H>
int image_check_sum(const void *buf, size_t size, const H &h, char *msg, size_t msg_cap) {
  const uint64_t sum = image_checksum(h, (const unsigned char *)buf + sizeof(H), size - sizeof(H));
  if (sum != h.checksum)
    return image_flaw(msg, msg_cap, "checksum %016llx, the bytes sum to %016llx (a damaged snapshot)", (unsigned long long)h.checksum, (unsigned long long)sum);
  return 0;
}

// the back of an image that is a header and n records of a vouched-for record_bytes (`count_name`: the header's name for n); *rec: the first
template <class H>
int image_open_back(const char *count_name, const void *buf, size_t size, const H &h, uint32_t n, const unsigned char **rec, char *msg, size_t msg_cap) {
  if (size != sizeof(H) + (size_t)n * h.record_bytes)
    return image_flaw(msg, msg_cap, "%zu bytes do not match %s x record_bytes (%zu + %u x %u)", size, count_name, sizeof(H), n, h.record_bytes);
  *rec = (const unsigned char *)buf + sizeof(H);
  return image_check_sum(buf, size, h, msg, msg_cap);
}

// the padding p[live .. end) behind an image's live bytes (`what`: "the files", "the rows") is zero
inline int image_check_padding(const char *what, const unsigned char *p, uint64_t live, uint64_t end, char *msg, size_t msg_cap) {
  for (uint64_t i = live; i < end; i++)
    if (p[i] != 0) return image_flaw(msg, msg_cap, "padding byte %llu behind %s is 0x%02x, not zero", (unsigned long long)(i - live), what, p[i]);
  return 0;
}

}  // namespace fsk
