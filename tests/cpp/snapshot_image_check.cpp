// snapshot_image_check.cpp -- the host-only validators of stream snapshots (csrc/fsk_snapshot_image.h: snap_image_open, the
// definition fskhip_snapshot_info_get, _stream_config, _concat and fskhip_restore_streams use) and of processor snapshots
// (csrc/fsk_processor_image.h: proc_image_open, fskhip_processor_snapshot_info_get's and fskhip_processor_restore's) as a
// stand-alone program, built with ASan + UBSan by tests/test_snapshot_cpu.py and tests/test_processor_snapshot_cpu.py.  No kernel
// and no HIP is linked.  stdin: one image per line, a kind letter ("S" stream, "P" processor), a blank and the image as hex ("-" for
// an empty one, "null" for no image at all), each copied into a heap block of exactly its size, at an odd address, so that a read
// behind the image or an aligned load is caught.  stdout: per image "0 n_streams precision per_stream_configs record_bytes" (S),
// "0 n_records rx_capacity payload_capacity record_bytes" (P) -- and, for both, the sum of the records' bytes through the view
// the validator returns -- or "-1 message".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "fsk_processor_image.h"
#include "fsk_snapshot_image.h"

namespace {

unsigned long long byte_sum(const unsigned char *p, size_t n) {
  unsigned long long s = 0;
  for (size_t i = 0; i < n; i++) s += p[i];
  return s;
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.size() < 3 || (line[0] != 'S' && line[0] != 'P') || line[1] != ' ') { std::fprintf(stderr, "no kind letter\n"); return 2; }
    std::string hex = line.substr(2);
    const bool null = hex == "null";
    if (null || hex == "-") hex.clear();
    if (hex.size() % 2) { std::fprintf(stderr, "odd hex\n"); return 2; }
    const size_t n = hex.size() / 2;
    unsigned char *block = (unsigned char *)std::malloc(n + 1);
    unsigned char *img = block + 1;
    for (size_t i = 0; i < n; i++) img[i] = (unsigned char)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
    char msg[512] = "";
    if (line[0] == 'S') {
      fsk::Snap s;
      if (fsk::snap_image_open(null ? nullptr : img, n, &s, msg, sizeof(msg)) != 0) std::printf("-1 %s\n", msg);
      else
        std::printf("0 %u %d %u %u %llu\n", s.h.n_streams, s.h.precision, s.h.per_stream_configs, s.h.record_bytes,
                    byte_sum(s.rec, (size_t)s.h.n_streams * s.h.record_bytes));
    } else {
      fsk::ProcSnap s;
      if (fsk::proc_image_open(null ? nullptr : img, n, &s, msg, sizeof(msg)) != 0) std::printf("-1 %s\n", msg);
      else
        std::printf("0 %u %u %u %u %llu\n", s.h.n_records, s.h.rx_capacity, s.h.payload_capacity, s.h.record_bytes,
                    byte_sum(s.rec, (size_t)s.h.n_records * s.h.record_bytes));
    }
    std::free(block);
  }
  return 0;
}
