// fsk_snapsum.h -- the checksum every image format of this library carries (stream, processor and XModem snapshots).  Host-only:
// no HIP, so that a format's validator can be compiled into a stand-alone check program.  Not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>
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

}  // namespace fsk
