// xmodem_snapshot_check.cpp -- the host-only validator of XModem snapshots (csrc/fsk_xmodem_image.h: xm_image_open, the definition
// fskhip_xmodem_snapshot_info_get and the three restores use) as a stand-alone program, built with ASan + UBSan by
// tests/test_xmodem_snapshot_cpu.py.  stdin: one image per line as hex ("-" for an empty one), each copied into a heap block of
// exactly its size, at an odd address, so that a read behind the image or an aligned load is caught.  stdout: per image
// "0 kind n_records param0 param1 file_bytes files_sum" -- files_sum adds every file byte through the view the validator returns --
// or "-1 message".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "fsk_xmodem_image.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line == "-") line.clear();
    if (line.size() % 2) { std::fprintf(stderr, "odd hex\n"); return 2; }
    const size_t n = line.size() / 2;
    unsigned char *block = (unsigned char *)std::malloc(n + 1);
    unsigned char *img = block + 1;
    for (size_t i = 0; i < n; i++) img[i] = (unsigned char)std::stoul(line.substr(2 * i, 2), nullptr, 16);
    fsk::XmImage im;
    char msg[256] = "";
    if (fsk::xm_image_open(img, n, &im, msg, sizeof(msg)) != 0) {
      std::printf("-1 %s\n", msg);
    } else {
      unsigned long long sum = 0, at = 0;
      for (uint32_t r = 0; r < im.h.n_records; r++) {
        for (uint32_t k = 0; k < im.file_len(r); k++) sum += im.files[at + k];
        at += im.file_len(r);
      }
      std::printf("0 %u %u %u %u %llu %llu\n", im.h.kind, im.h.n_records, im.h.param0, im.h.param1, (unsigned long long)im.h.file_bytes, sum);
    }
    std::free(block);
  }
  // a null image and one shorter than a header
  fsk::XmImage im;
  char msg[256] = "";
  if (fsk::xm_image_open(nullptr, 0, &im, msg, sizeof(msg)) == 0) return 3;
  std::printf("-1 %s\n", msg);
  return 0;
}
