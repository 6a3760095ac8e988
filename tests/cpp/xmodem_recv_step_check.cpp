// The resident XModem file receiver's transition (webaudio_modem_amd/csrc/fsk_xmodem_recv_step.h) and the one-reply mode of the
// receive grammar (fsk_xmodem_scan.h) as a host program: the same text the step kernel compiles for the device, over cases read
// from stdin.  One case per line:
//   <state> <expected> <retries> <file_len> <abort> <pending> <timeout> <max_retries> <file_capacity> <hex ring bytes or ->
// The bytes are walked oldest first while no reply is owed, as the kernel walks a ring.  Output: one line per case -- the event's
// twelve words, then touched, listed, removed, span, appended, and the increase of packets_received, dropped and packets_sent.
// Built by tests/test_xmodem_recv_cpu.py with -fsanitize=address,undefined.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "fsk_xmodem_recv_step.h"

using namespace fsk;

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

int main() {
  uint32_t table[256];
  for (uint32_t i = 0; i < 256u; i++) table[i] = xm::crc_table_entry(i);
  unsigned state, expected, retries, file_len, abort_, pending, timeout, max_retries, file_capacity;
  std::string hex;
  while (std::cin >> state >> expected >> retries >> file_len >> abort_ >> pending >> timeout >> max_retries >> file_capacity >> hex) {
    std::vector<uint8_t> in;
    if (hex != "-") {
      if (hex.size() % 2) { std::fprintf(stderr, "odd hex string\n"); return 2; }
      for (size_t i = 0; i < hex.size(); i += 2) {
        const int hi = nibble(hex[i]), lo = nibble(hex[i + 1]);
        if (hi < 0 || lo < 0) { std::fprintf(stderr, "bad hex digit\n"); return 2; }
        in.push_back((uint8_t)(hi * 16 + lo));
      }
    }
    if (state == FSKHIP_XR_IDLE || state > FSKHIP_XR_SEND_ACK || expected < 1u || expected > 255u || file_len > file_capacity) {
      std::fprintf(stderr, "bad case\n");
      return 2;
    }
    const bool look = !abort_ && !pending;
    const uint32_t n = look ? (uint32_t)in.size() : 0u;
    xm::Scan sc;
    sc.init(look ? expected : 1u);
    for (uint32_t pos = 0; pos < n && !sc.owes_reply(); pos++) sc.byte<false>(table, in[pos], pos, nullptr, 0);
    xr::Words W{state, expected, retries, file_len, 0u, 0u, 0u};
    const xr::Step R = xr::step(W, abort_ != 0, pending != 0, look && timeout != 0, xr::found_of(sc), n, max_retries, file_capacity);
    if (R.appended && (R.span + R.ev.accepted_len > n || R.ev.file_len > file_capacity)) { std::fprintf(stderr, "span out of bounds\n"); return 3; }
    if (R.removed > n) { std::fprintf(stderr, "removed out of bounds\n"); return 3; }
    std::printf("%u %u %d %u %d %d %u %u %u %u %d %d %u %u %u %u %u %u %u %u\n", R.ev.status, R.ev.state_after, R.ev.control, R.ev.step, R.ev.seq, R.ev.len,
                R.ev.accepted_len, R.ev.file_len, R.ev.expected, R.ev.retries, R.ev.crc_rx, R.ev.crc_calc, R.touched, R.listed, R.removed, R.span, R.appended,
                W.packets, W.dropped, W.sent);
  }
  return 0;
}
