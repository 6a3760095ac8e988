// resample_image_check.cpp -- the host-only validator of resampler snapshots (csrc/fsk_resample_image.h: rs_image_open, the
// definition fskhip_resampler_snapshot_info_get and fskhip_resampler_restore use) as a stand-alone program, built with ASan + UBSan
// by tests/test_resample_remap_cpu.py.  No kernel and no HIP is linked.
//
// Part one, stdin: one image per line as hex ("-" for an empty one), each copied into a heap block of exactly its size, at an odd
// address, so that a read behind the image or an aligned load is caught.  stdout: per image
// "0 n_records direction factor n_taps precision history taps_sum rows_sum" -- the sums run over the views the validator returns,
// the rows as bytes -- or "-1 message".
// Part two: images built here from the header's own layout, and every damage the format knows, each checked against the text its
// flaw must carry; "case <name> ok" per case, exit status 1 and "case <name> FAILED: ..." otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "fsk_resample_image.h"

namespace {

using Bytes = std::vector<unsigned char>;

void seal(Bytes &b) {   // the checksum over the image as it stands
  fsk::RsImageHeader h;
  std::memcpy(&h, b.data(), sizeof(h));
  fsk::image_seal(h, b.data(), b.size());
}

// a well-formed image; `tweak` changes the header before the body is laid out by ITS numbers and the checksum is made
template <class Tweak>
Bytes build(uint32_t direction, uint32_t factor, uint32_t n_taps, uint32_t n_records, Tweak tweak, bool reseal = true) {
  fsk::RsImageHeader h = fsk::image_header<fsk::RsImageHeader>(fsk::kRsMagic, fsk::kRsFormat);
  h.n_records = n_records; h.direction = direction; h.factor = factor; h.n_taps = n_taps; h.precision = 0;
  h.history = fsk::resample_history((int)direction, factor, n_taps);
  h.record_bytes = 4u * h.history;
  const uint32_t hist = h.history;
  tweak(h);
  Bytes b((size_t)fsk::rs_image_bytes(n_records, n_taps, hist), 0);
  std::memcpy(b.data(), &h, sizeof(h));
  for (uint32_t i = 0; i < n_taps; i++) {
    const double t = 0.25 + i;
    std::memcpy(b.data() + sizeof(h) + 8u * (size_t)i, &t, 8);
  }
  for (size_t i = 0; i < (size_t)n_records * hist; i++) {
    const uint32_t w = 0x7FC00000u + (uint32_t)i;   // NaNs with a payload: any word is a valid history word
    std::memcpy(b.data() + sizeof(h) + 8u * (size_t)n_taps + 4u * i, &w, 4);
  }
  if (reseal) seal(b);
  return b;
}
Bytes good(uint32_t direction = 0, uint32_t factor = 2, uint32_t n_taps = 6, uint32_t n_records = 3) {
  return build(direction, factor, n_taps, n_records, [](fsk::RsImageHeader &) {});
}

int open_at_odd_address(const unsigned char *data, size_t n, fsk::RsImage *im, unsigned char **block, char *msg, size_t cap) {
  *block = (unsigned char *)std::malloc(n + 1);
  if (n) std::memcpy(*block + 1, data, n);
  return fsk::rs_image_open(*block + 1, n, im, msg, cap);
}

int failures = 0;
void expect(const char *name, const Bytes &b, const char *want) {   // want: a part of the flaw's text, or null for a valid image
  fsk::RsImage im;
  unsigned char *block = nullptr;
  char msg[256] = "";
  const int rc = open_at_odd_address(b.data(), b.size(), &im, &block, msg, sizeof(msg));
  const bool ok = want ? (rc == -1 && std::strstr(msg, want) != nullptr) : rc == 0;
  if (ok) std::printf("case %s ok\n", name);
  else { std::printf("case %s FAILED: rc %d, \"%s\", wanted %s\n", name, rc, msg, want ? want : "a valid image"); failures++; }
  std::free(block);
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line == "-") line.clear();
    if (line.size() % 2) { std::fprintf(stderr, "odd hex\n"); return 2; }
    Bytes img(line.size() / 2);
    for (size_t i = 0; i < img.size(); i++) img[i] = (unsigned char)std::stoul(line.substr(2 * i, 2), nullptr, 16);
    fsk::RsImage im;
    unsigned char *block = nullptr;
    char msg[256] = "";
    if (open_at_odd_address(img.data(), img.size(), &im, &block, msg, sizeof(msg)) != 0) {
      std::printf("-1 %s\n", msg);
    } else {
      double taps = 0;
      for (uint32_t i = 0; i < im.h.n_taps; i++) taps += im.tap(i);
      unsigned long long rows = 0;
      for (size_t i = 0; i < (size_t)im.h.n_records * im.h.record_bytes; i++) rows += im.rows[i];
      std::printf("0 %u %u %u %u %u %u %.17g %llu\n", im.h.n_records, im.h.direction, im.h.factor, im.h.n_taps, im.h.precision, im.h.history, taps, rows);
    }
    std::free(block);
  }

  // ---- part two ----
  const size_t H = sizeof(fsk::RsImageHeader);
  {
    fsk::RsImage im;
    char msg[256] = "";
    if (fsk::rs_image_open(nullptr, 0, &im, msg, sizeof(msg)) == 0 || !std::strstr(msg, "null snapshot")) { std::printf("case null FAILED\n"); failures++; }
    else std::printf("case null ok\n");
  }
  // valid: both directions, the designs of the device tests, no records, no history
  expect("good-up", good(0, 2, 6, 3), nullptr);
  expect("good-down", good(1, 2, 6, 3), nullptr);
  expect("good-default-up", good(0, 6, 97, 5), nullptr);
  expect("good-default-down", good(1, 6, 97, 2), nullptr);
  expect("good-no-history", good(0, 1, 1, 7), nullptr);
  expect("good-no-records", good(1, 3, 13, 0), nullptr);
  expect("good-longest", good(1, 1, 4096, 1), nullptr);
  // truncation at every header boundary (each field's start), and within the taps, the rows and the padding
  const Bytes g = good();
  for (size_t cut = 0; cut < H; cut += 4) {
    const std::string name = "cut-header-" + std::to_string(cut);
    expect(name.c_str(), Bytes(g.begin(), g.begin() + (long)cut), "fewer than a resampler snapshot header");
  }
  expect("cut-at-header", Bytes(g.begin(), g.begin() + (long)H), "do not match the layout");
  expect("cut-in-taps", Bytes(g.begin(), g.begin() + (long)(H + 8)), "do not match the layout");
  expect("cut-at-taps", Bytes(g.begin(), g.begin() + (long)(H + 48)), "do not match the layout");
  expect("cut-in-rows", Bytes(g.begin(), g.begin() + (long)(H + 48 + 16)), "do not match the layout");
  expect("cut-padding", Bytes(g.begin(), g.end() - 16), "do not match the layout");
  {
    Bytes b = g;
    b.insert(b.end(), 16, 0);
    expect("overlong", b, "do not match the layout");
  }
  // a flipped byte in header, taps, body and padding (the image is 48 + 48 + 36 bytes and 12 of padding)
  const size_t flips[][1] = {{17}, {H + 5}, {H + 48 + 7}, {H + 48 + 36 + 3}};
  const char *flip_names[] = {"flip-header", "flip-taps", "flip-rows", "flip-padding"};
  for (int i = 0; i < 4; i++) {
    Bytes b = g;
    b[flips[i][0]] ^= 0x40;
    expect(flip_names[i], b, i == 0 ? "n_records" : "checksum");   // (byte 17 is n_records: the size no longer fits)
  }
  {
    Bytes b = g;
    b[40] ^= 1;   // the checksum itself
    expect("flip-checksum", b, "checksum");
  }
  expect("magic", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.magic = 0x584B5346u; }), "not a resampler snapshot");
  expect("format", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.format = 2; }), "format 2");
  expect("header-bytes", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.header_bytes = 64; }), "header_bytes 64");
  expect("direction", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.direction = 2; }), "direction 2");
  expect("precision", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.precision = 2; }), "precision 2");
  expect("record-count-more", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.n_records = 5; }), "do not match the layout");
  expect("record-count-fewer", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.n_records = 1; }), "do not match the layout");
  expect("record-count-huge", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.n_records = 0xFFFFFFFFu; }), "do not match the layout");
  expect("history-of-the-other-direction", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.history = 5; h.record_bytes = 20; }), "history 5");
  expect("history-off-by-one", build(1, 2, 6, 3, [](fsk::RsImageHeader &h) { h.history = 4; h.record_bytes = 16; }), "history 4");
  expect("record-bytes", build(1, 2, 6, 3, [](fsk::RsImageHeader &h) { h.record_bytes = 24; }), "record_bytes 24");
  expect("factor-0", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.factor = 0; }), "factor 0 outside 1..32");
  expect("factor-33", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.factor = 33; }), "factor 33 outside 1..32");
  expect("taps-0", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.n_taps = 0; }), "n_taps 0 outside 1..4096");
  expect("taps-4097", build(0, 2, 6, 3, [](fsk::RsImageHeader &h) { h.n_taps = 4097; }), "n_taps 4097 outside 1..4096");
  {
    Bytes b = g;   // non-zero padding under a checksum that matches
    b[b.size() - 2] = 1;
    seal(b);
    expect("padding", b, "padding byte 10");
  }
  return failures ? 1 : 0;
}
