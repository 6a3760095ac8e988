// xmodem_timer_image_check.cpp -- the host-only validator of XModem timer snapshots (csrc/fsk_xmodem_timer_image.h: xw_image_open,
// the definition fskhip_xmodem_timer_snapshot_info_get and fskhip_xmodem_timer_restore use) as a stand-alone program, built with
// ASan + UBSan by tests/test_xmodem_timer_image_cpu.py.  It writes a 5-record image of each kind with fsk_image.h's header and seal
// (an odd count: 8 bytes of padding), has the validator accept it and read every record back, and then hands it every truncation
// of the image and every single-byte corruption of it (each byte set to each of the 255 other values).  None may be accepted.
// Every candidate is copied into a heap block of exactly its size, at an odd address, so that a read behind the image or an
// aligned load is caught.  stdout: the flaws' texts of the truncations, then "<n> expectations, <m> failed".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fsk_xmodem_timer_image.h"

namespace {

int expectations = 0, failed = 0;

void expect(bool ok, const char *what, size_t at, unsigned value) {
  expectations++;
  if (!ok) {
    failed++;
    std::printf("FAILED: %s (at %zu, value %u)\n", what, at, value);
  }
}

// the validator over a copy of exactly n bytes at an odd address
int open_copy(const unsigned char *bytes, size_t n, fsk::XwImage *im, const unsigned char **copy, unsigned char **block, char *msg, size_t msg_cap) {
  *block = (unsigned char *)std::malloc(n + 1);
  unsigned char *img = *block + 1;
  if (n) std::memcpy(img, bytes, n);
  *copy = img;
  return fsk::xw_image_open(img, n, im, msg, msg_cap);
}

std::vector<unsigned char> image(uint32_t kind, const std::vector<fsk::xw::Words> &records, uint32_t timeout_samples) {
  fsk::XwImageHeader h = fsk::image_header<fsk::XwImageHeader>(fsk::kXwMagic, fsk::kXwFormat);
  h.kind = kind; h.n_records = (uint32_t)records.size(); h.record_words = fsk::kXwRecordWords; h.timeout_samples = timeout_samples;
  std::vector<unsigned char> out((size_t)fsk::xw_image_bytes(h.n_records), 0);
  for (size_t r = 0; r < records.size(); r++) {
    std::memcpy(&out[sizeof(h) + 8 * r], &records[r].waited, 4);
    std::memcpy(&out[sizeof(h) + 8 * r + 4], &records[r].mark, 4);
  }
  fsk::image_seal(h, out.data(), out.size());
  return out;
}

void walk(uint32_t kind, const std::vector<fsk::xw::Words> &records) {
  const std::vector<unsigned char> good = image(kind, records, 12288u);
  expect(good.size() == 96, "a 5-record image has 96 bytes", good.size(), 0);
  fsk::XwImage im;
  const unsigned char *copy;
  unsigned char *block;
  char msg[256] = "";
  // accepted as it is, and every record reads back through the view
  expect(open_copy(good.data(), good.size(), &im, &copy, &block, msg, sizeof(msg)) == 0, msg, 0, kind);
  expect(im.h.kind == kind && im.h.n_records == records.size() && im.h.timeout_samples == 12288u, "the header as written", 0, kind);
  for (uint32_t r = 0; r < records.size(); r++)
    expect(im.record(r).waited == records[r].waited && im.record(r).mark == records[r].mark, "a record as written", r, kind);
  std::free(block);
  // every truncation
  for (size_t n = 0; n < good.size(); n++) {
    msg[0] = 0;
    const int rc = open_copy(good.data(), n, &im, &copy, &block, msg, sizeof(msg));
    expect(rc != 0 && msg[0] != 0, "a truncated image is refused with a message", n, kind);
    if (n % 8 == 0) std::printf("%u: %zu bytes: %s\n", kind, n, msg);
    std::free(block);
  }
  // every single-byte corruption
  std::vector<unsigned char> bad = good;
  for (size_t at = 0; at < good.size(); at++) {
    for (unsigned v = 0; v < 256; v++) {
      if (v == good[at]) continue;
      bad[at] = (unsigned char)v;
      msg[0] = 0;
      const int rc = open_copy(bad.data(), bad.size(), &im, &copy, &block, msg, sizeof(msg));
      expect(rc != 0 && msg[0] != 0, "a corrupted image is refused with a message", at, v);
      std::free(block);
    }
    bad[at] = good[at];
  }
}

}  // namespace

int main() {
  walk(fsk::kXwKindRecv, {{0u, 0u}, {1u, 1u}, {12287u, 2u}, {12288u, 6u}, {0xFFFFFFFFu, 4u}});
  walk(fsk::kXwKindTx, {{0u, 0u}, {1u, 4u}, {8191u, 0u}, {8192u, 4u}, {0xFFFFFFFFu, 0u}});
  // a null image
  fsk::XwImage im;
  char msg[256] = "";
  expect(fsk::xw_image_open(nullptr, 0, &im, msg, sizeof(msg)) != 0 && msg[0] != 0, "a null image is refused", 0, 0);
  std::printf("%d expectations, %d failed\n", expectations, failed);
  return failed ? 1 : 0;
}
