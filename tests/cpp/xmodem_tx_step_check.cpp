// The resident XModem sender's transition (webaudio_modem_amd/csrc/fsk_xmodem_tx_step.h) as a host program: the same text the
// step kernel compiles for the device, over cases read from stdin.  One case per line:
//   <state> <sequence> <fragment_index> <retries> <abort> <pending> <max_retries> <file_len> <max_payload> <skew> <hex reply or ->
// The reply is searched as the kernel searches a ring: skew 0..15 places it at bytes [skew, skew + n) of a sequence of 16-byte
// quads, walked in tiles of four quads until the wait is settled; skew 16 feeds it byte by byte.  Output: one line per case --
// the event's eight words, then send, touched, drained, listed, and the increase of packets_sent and retransmitted.  If the packet
// is built on the device its bytes are not this program's business: the header only decides.  Built by tests/test_xmodem_tx_cpu.py
// with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "fsk_xmodem_tx_step.h"

using namespace fsk::xt;

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

int main() {
  unsigned state, sequence, index, retries, abort_, pending, max_retries, file_len, max_payload, skew;
  std::string hex;
  while (std::cin >> state >> sequence >> index >> retries >> abort_ >> pending >> max_retries >> file_len >> max_payload >> skew >> hex) {
    std::vector<uint8_t> in;
    if (hex != "-") {
      if (hex.size() % 2) { std::fprintf(stderr, "odd hex string\n"); return 2; }
      for (size_t i = 0; i < hex.size(); i += 2) {
        const int hi = nibble(hex[i]), lo = nibble(hex[i + 1]);
        if (hi < 0 || lo < 0) { std::fprintf(stderr, "bad hex digit\n"); return 2; }
        in.push_back((uint8_t)(hi * 16 + lo));
      }
    }
    if (state == FSKHIP_XT_IDLE || max_payload < 1u || max_payload > 255u || skew > 16u) { std::fprintf(stderr, "bad case\n"); return 2; }
    const uint32_t n = (uint32_t)in.size();
    Find F;
    F.init();
    if (!abort_ && !pending) {
      if (skew == 16u) {
        for (uint32_t pos = 0; pos < n && !F.settled(state); pos++) F.byte(in[pos]);
      } else {
        const uint32_t need = n ? skew + n : 0u;
        std::vector<uint8_t> quads(((size_t)need + 15u) / 16u * 16u, 0xEE);   // exactly the quads the kernel would load
        if (n) std::memcpy(quads.data() + skew, in.data(), n);
        for (uint32_t t0 = 0; t0 < need && !F.settled(state); t0 += 64u) {
          for (uint32_t c = 0; c < 4u; c++) {
            const uint32_t at = t0 + 16u * c;
            if (at >= need || F.settled(state)) break;
            uint32_t w[4];
            std::memcpy(w, quads.data() + at, 16);   // (little-endian host, as the device)
            const uint32_t lo = at < skew ? skew - at : 0u, hi = need - at < 16u ? need - at : 16u;
            F.quad(w, lo < 16u ? lo : 16u, hi);
          }
        }
      }
    }
    Words W{state, sequence, index, fragment_count(file_len, max_payload), retries, 0u, 0u};
    const Step R = step(W, abort_ != 0, pending != 0, F, max_retries, file_len, max_payload);
    std::printf("%u %u %d %u %u %u %u %u %u %u %u %u %u %u\n", R.ev.status, R.ev.state_after, R.ev.control, R.ev.sent_len, R.ev.sequence, R.ev.fragment_index,
                R.ev.n_fragments, R.ev.retries, R.send, R.touched, R.drained, R.listed, W.sent, W.retransmitted);
  }
  return 0;
}
