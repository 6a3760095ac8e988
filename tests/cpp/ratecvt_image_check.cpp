// ratecvt_image_check.cpp -- the host-only validator of rate converter snapshots (csrc/fsk_ratecvt_image.h: rc_image_open, the
// definition fskhip_ratecvt_snapshot_info_get and fskhip_ratecvt_restore use) as a stand-alone program, built with ASan + UBSan
// by tests/test_ratecvt_remap_cpu.py.  No kernel and no HIP is linked.
//
// Part one, stdin: one image per line as hex ("-" for an empty one), each copied into a heap block of exactly its size, at an odd
// address, so that a read behind the image or an aligned load is caught.  stdout: per image
// "0 n_records direction up down n_taps precision history position taps_sum rows_sum" -- the sums run over the views the validator
// returns, the rows as bytes -- or "-1 message".
// Part two: images built here from the header's own layout functions, and every damage the format knows, each checked against
// the text its flaw must carry; then the order of refusals: images with two flaws are refused for the one that comes first.
// "case <name> ok" per case, exit status 1 and "case <name> FAILED: ..." otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "fsk_ratecvt_image.h"
#include "fsk_resample_image.h"

namespace {

using Bytes = std::vector<unsigned char>;
using Header = fsk::RcImageHeader;

void seal(Bytes &b) {   // the checksum over the image as it stands
  Header h;
  std::memcpy(&h, b.data(), sizeof(h));
  fsk::image_seal(h, b.data(), b.size());
}

// a well-formed image; `tweak` changes the header before the body is laid out by ITS numbers and the checksum is made
template <class Tweak>
Bytes build(uint32_t direction, uint32_t up, uint32_t down, uint32_t n_taps, uint32_t n_records, uint32_t position, Tweak tweak) {
  Header h = fsk::image_header<Header>(fsk::kRcMagic, fsk::kRcFormat);
  h.n_records = n_records; h.direction = direction; h.up = up; h.down = down; h.n_taps = n_taps; h.precision = 0;
  h.history = fsk::resample_history(0, up, n_taps);
  h.position = position;
  h.record_bytes = 4u * h.history;
  const uint32_t hist = h.history;
  tweak(h);
  Bytes b((size_t)fsk::rc_image_bytes(n_records, n_taps, hist), 0);
  std::memcpy(b.data(), &h, sizeof(h));
  for (uint32_t i = 0; i < n_taps; i++) {
    const double t = 0.25 + i;
    std::memcpy(b.data() + sizeof(h) + 8u * (size_t)i, &t, 8);
  }
  for (size_t i = 0; i < (size_t)n_records * hist; i++) {
    const uint32_t w = 0x7FC00000u + (uint32_t)i;   // NaNs with a payload: any word is a valid history word
    std::memcpy(b.data() + sizeof(h) + 8u * (size_t)n_taps + 4u * i, &w, 4);
  }
  seal(b);
  return b;
}
Bytes good(uint32_t direction = 0, uint32_t up = 2, uint32_t down = 3, uint32_t n_taps = 6, uint32_t n_records = 3, uint32_t position = 2) {
  return build(direction, up, down, n_taps, n_records, position, [](Header &) {});
}
template <class Tweak>
Bytes bad(Tweak tweak) { return build(0, 2, 3, 6, 3, 2, tweak); }

// a resampler's image, written by ITS layout functions: the stranger a converter is likeliest to meet
Bytes resampler_image() {
  fsk::RsImageHeader h = fsk::image_header<fsk::RsImageHeader>(fsk::kRsMagic, fsk::kRsFormat);
  h.n_records = 3; h.direction = 0; h.factor = 2; h.n_taps = 6; h.precision = 0;
  h.history = fsk::resample_history(0, 2, 6);
  h.record_bytes = 4u * h.history;
  Bytes b((size_t)fsk::rs_image_bytes(3, 6, h.history), 0);
  fsk::image_seal(h, b.data(), b.size());
  return b;
}

int open_at_odd_address(const unsigned char *data, size_t n, fsk::RcImage *im, unsigned char **block, char *msg, size_t cap) {
  *block = (unsigned char *)std::malloc(n + 1);
  if (n) std::memcpy(*block + 1, data, n);
  return fsk::rc_image_open(*block + 1, n, im, msg, cap);
}

int failures = 0;
void expect(const char *name, const Bytes &b, const char *want) {   // want: a part of the flaw's text, or null for a valid image
  fsk::RcImage im;
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
    fsk::RcImage im;
    unsigned char *block = nullptr;
    char msg[256] = "";
    if (open_at_odd_address(img.data(), img.size(), &im, &block, msg, sizeof(msg)) != 0) {
      std::printf("-1 %s\n", msg);
    } else {
      double taps = 0;
      for (uint32_t i = 0; i < im.h.n_taps; i++) taps += im.tap(i);
      unsigned long long rows = 0;
      for (size_t i = 0; i < (size_t)im.h.n_records * im.h.record_bytes; i++) rows += im.rows[i];
      std::printf("0 %u %u %u %u %u %u %u %u %.17g %llu\n", im.h.n_records, im.h.direction, im.h.up, im.h.down, im.h.n_taps, im.h.precision, im.h.history,
                  im.h.position, taps, rows);
    }
    std::free(block);
  }

  // ---- part two ----
  const size_t H = sizeof(Header);
  {
    fsk::RcImage im;
    char msg[256] = "";
    if (fsk::rc_image_open(nullptr, 0, &im, msg, sizeof(msg)) == 0 || !std::strstr(msg, "null snapshot")) { std::printf("case null FAILED\n"); failures++; }
    else std::printf("case null ok\n");
  }
  // valid: both directions, the designs of the device tests, no records, no history, the longest row, the last position
  expect("good-capture", good(0, 2, 3, 6, 3, 2), nullptr);
  expect("good-playback", good(1, 3, 2, 13, 3, 1), nullptr);
  expect("good-default-capture", good(0, 160, 147, 2561, 5, 146), nullptr);
  expect("good-default-playback", good(1, 147, 160, 2561, 2, 159), nullptr);
  expect("good-no-history", good(0, 1, 1, 1, 7, 0), nullptr);
  expect("good-no-records", good(1, 3, 2, 13, 0, 0), nullptr);
  expect("good-longest", good(1, 1, 256, 4096, 1, 255), nullptr);
  // truncation at every header boundary (each field's start), and within the taps, the rows and the padding
  const Bytes g = good();
  for (size_t cut = 0; cut < H; cut += 4) {
    const std::string name = "cut-header-" + std::to_string(cut);
    expect(name.c_str(), Bytes(g.begin(), g.begin() + (long)cut), "fewer than a rate converter snapshot header");
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
  // a flipped byte in header, taps, body and padding (the image is 64 + 48 + 36 bytes and 12 of padding)
  const size_t flips[] = {17, H + 5, H + 48 + 7, H + 48 + 36 + 3};
  const char *flip_names[] = {"flip-header", "flip-taps", "flip-rows", "flip-padding"};
  for (int i = 0; i < 4; i++) {
    Bytes b = g;
    b[flips[i]] ^= 0x40;
    expect(flip_names[i], b, i == 0 ? "n_records" : "checksum");   // (byte 17 is n_records: the size no longer fits)
  }
  {
    Bytes b = g;
    b[offsetof(Header, checksum)] ^= 1;   // the checksum itself
    expect("flip-checksum", b, "checksum");
  }
  // every header field, by itself
  expect("magic", bad([](Header &h) { h.magic = 0x584B5346u; }), "not a rate converter snapshot (magic 0x584b5346");
  expect("magic-resampler", resampler_image(), "is a resampler snapshot's");
  {
    const Bytes r = resampler_image();
    expect("resampler-truncated", Bytes(r.begin(), r.begin() + 48), "fewer than a rate converter snapshot header");
  }
  expect("format", bad([](Header &h) { h.format = 2; }), "format 2");
  expect("header-bytes", bad([](Header &h) { h.header_bytes = 48; }), "header_bytes 48");
  expect("reserved-0", bad([](Header &h) { h.reserved[0] = 1; }), "reserved words");
  expect("reserved-1", bad([](Header &h) { h.reserved[1] = 0x80000000u; }), "reserved words");
  expect("direction", bad([](Header &h) { h.direction = 2; }), "direction 2");
  expect("up-0", bad([](Header &h) { h.up = 0; }), "up 0 outside 1..256");
  expect("up-257", bad([](Header &h) { h.up = 257; }), "up 257 outside 1..256");
  expect("down-0", bad([](Header &h) { h.down = 0; }), "down 0 outside 1..256");
  expect("down-257", bad([](Header &h) { h.down = 257; }), "down 257 outside 1..256");
  expect("lowest-terms", bad([](Header &h) { h.down = 4; }), "2 / 4 is not in lowest terms");
  expect("taps-0", bad([](Header &h) { h.n_taps = 0; }), "n_taps 0 outside 1..4096");
  expect("taps-4097", bad([](Header &h) { h.n_taps = 4097; }), "n_taps 4097 outside 1..4096");
  expect("precision", bad([](Header &h) { h.precision = 2; }), "precision 2");
  expect("history-of-a-decimator", bad([](Header &h) { h.history = 5; h.record_bytes = 20; }), "history 5, 6 taps at an up factor of 2 keep 3");
  expect("history-off-by-one", bad([](Header &h) { h.history = 2; h.record_bytes = 8; }), "history 2");
  expect("position-at-down", bad([](Header &h) { h.position = 3; }), "position 3 is not below the down factor 3");
  expect("position-huge", bad([](Header &h) { h.position = 0xFFFFFFFFu; }), "position 4294967295");
  expect("record-bytes", bad([](Header &h) { h.record_bytes = 16; }), "record_bytes 16, a row of 3 floats has 12");
  expect("record-count-more", bad([](Header &h) { h.n_records = 5; }), "do not match the layout");
  expect("record-count-fewer", bad([](Header &h) { h.n_records = 1; }), "do not match the layout");
  expect("record-count-huge", bad([](Header &h) { h.n_records = 0xFFFFFFFFu; }), "do not match the layout");
  {
    Bytes b = g;   // non-zero padding under a checksum that matches
    b[b.size() - 2] = 1;
    seal(b);
    expect("padding", b, "padding byte 10");
  }
  // the order of refusals: each image has the flaw named and EVERY flaw behind it in the documented order; the first is the one named
  {
    struct Step { const char *name; void (*damage)(Header &); const char *want; };
    const Step steps[] = {
        {"magic", [](Header &h) { h.magic ^= 1u; }, "not a rate converter snapshot"},
        {"format", [](Header &h) { h.format = 9; }, "format 9"},
        {"header-bytes", [](Header &h) { h.header_bytes = 80; }, "header_bytes 80"},
        {"reserved", [](Header &h) { h.reserved[0] = 7; }, "reserved words"},
        {"direction", [](Header &h) { h.direction = 3; }, "direction 3"},
        {"up", [](Header &h) { h.up = 300; }, "up 300"},
        {"down", [](Header &h) { h.down = 0; }, "down 0"},
        {"taps", [](Header &h) { h.n_taps = 5000; }, "n_taps 5000"},
        {"precision", [](Header &h) { h.precision = 4; }, "precision 4"},
        {"history", [](Header &h) { h.history += 1; }, "history "},
        {"position", [](Header &h) { h.position = 1000; }, "position 1000"},
        {"record-bytes", [](Header &h) { h.record_bytes += 4; }, "record_bytes "},
    };
    const size_t n = sizeof(steps) / sizeof(steps[0]);
    for (size_t first = 0; first < n; first++) {
      Bytes b = g;
      Header h;
      std::memcpy(&h, b.data(), sizeof(h));
      for (size_t k = n; k-- > first;) {
        // (up 300 and down 0 would hide what follows only by coming first, which is the point; history is damaged against the
        // design the header then names, so it is a flaw whatever up and n_taps have become)
        steps[k].damage(h);
      }
      std::memcpy(b.data(), &h, sizeof(h));
      b.resize(b.size() - 16);                 // ... the size against the layout,
      b[b.size() - 1] = 1;                     // the padding
      b[offsetof(Header, checksum)] ^= 0x55;   // and the checksum are wrong in every one of them
      const std::string name = std::string("order-") + steps[first].name;
      expect(name.c_str(), b, steps[first].want);
    }
    // behind the header's words: the size, then the checksum, then the padding
    Bytes b = g;
    b[b.size() - 2] = 1;                       // padding damaged, checksum stale, 16 bytes short
    b.resize(b.size() - 16);
    expect("order-size", b, "do not match the layout");
    b = g;
    b[b.size() - 2] = 1;                       // padding damaged and the checksum stale
    expect("order-checksum", b, "checksum");
  }
  return failures ? 1 : 0;
}
