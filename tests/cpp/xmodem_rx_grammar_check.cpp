// The receive grammar's shared state machine (webaudio_modem_amd/csrc/fsk_xmodem_scan.h) as a host program: the same code the
// burst scan and the resident receiver compile for the device, over cases read from stdin.  One case per line:
//   B <expected> <hex bytes or ->   a recorded burst  (Scan::finish)            -> ten result words, 0, the assembled payload
//   S <expected> <hex bytes or ->   a live line so far (Scan::finish_streaming) -> ten result words, the bytes that leave, payload
// Output: one line per case, the words in decimal, the payload in hex ("-" when empty).  Built by tests/test_xmodem_rx_cpu.py
// with -fsanitize=address,undefined.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "fsk_xmodem_scan.h"

using namespace fsk::xm;

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

int main() {
  uint32_t table[256];
  for (uint32_t i = 0; i < 256; i++) table[i] = crc_table_entry(i);
  std::string mode, hex;
  unsigned expected;
  while (std::cin >> mode >> expected >> hex) {
    std::vector<uint8_t> in;
    if (hex != "-") {
      if (hex.size() % 2) { std::fprintf(stderr, "odd hex string\n"); return 2; }
      for (size_t i = 0; i < hex.size(); i += 2) {
        const int hi = nibble(hex[i]), lo = nibble(hex[i + 1]);
        if (hi < 0 || lo < 0) { std::fprintf(stderr, "bad hex digit\n"); return 2; }
        in.push_back((uint8_t)(hi * 16 + lo));
      }
    }
    const uint32_t n = (uint32_t)in.size();
    std::vector<uint8_t> data(n + 4u, 0);   // the assembled payload is never longer than the input
    Scan sc;
    sc.init(expected);
    for (uint32_t pos = 0; pos < n && sc.state != ST_DONE; pos++) sc.byte<false>(table, in[pos], pos, data.data(), data.size());
    fskhip_xmodem_result r;
    uint32_t removed = 0;
    if (mode == "B") sc.finish(&r);
    else if (mode == "S") removed = sc.finish_streaming(&r, n);
    else { std::fprintf(stderr, "unknown mode\n"); return 2; }
    std::printf("%u %u %u %u %u %u %d %d %d %d %u ", r.status, r.expected_after, r.packets, r.dropped, r.consumed, r.data_len, r.err_seq, r.err_len, r.crc_rx,
                r.crc_calc, removed);
    if (r.data_len == 0) std::printf("-");
    for (uint32_t i = 0; i < r.data_len; i++) std::printf("%02x", data[i]);
    std::printf("\n");
  }
  return 0;
}
