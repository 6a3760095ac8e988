// fsk_xmodem_tx_step.h -- XModemTransport's send side as one transition per demodulate() reply, defined once: the resident
// sender's step kernel (fsk_xmodem_tx.hip) and a host program (tests/cpp/xmodem_tx_step_check.cpp) include the same text.  What it
// restates: sendData's three waits, src/transports/xmodem/xmodem.ts:109-184, 389-470, 602-628 -- what each wait does with ONE
// reply of the data channel -- pinned to the real class by tests/golden/golden_xmodem_tx.npz.  The contract is in
// include/fskhip_next.h.  Plain C++ as well as HIP (FSK_XT_FN is plain `inline` without a device compiler).  Not part of the ABI.
#pragma once
#include <stdint.h>

#include "../../include/fskhip_next.h"
#include "fsk_xmodem_scan.h"

#if defined(__HIPCC__)
#define FSK_XT_FN __host__ __device__ __forceinline__   // (the C-ABI unit counts fragments on the host with the same functions)
#else
#define FSK_XT_FN inline
#endif

namespace fsk {
namespace xt {

constexpr uint32_t kACK = 0x06, kNAK = 0x15, kEOT = 0x04;   // types.ts:29-34
enum : uint32_t { SEND_NOTHING = 0, SEND_PACKET = 1, SEND_EOT = 2 };

// what the two waits look for in a reply: waitForControlByte returns the FIRST of ACK / NAK / EOT (xmodem.ts:413-418) and the
// rest of the reply is lost; waitForACK succeeds on an ACK ANYWHERE (xmodem.ts:448-452).  Bytes are fed oldest first.
struct Find {
  int32_t first;   // the first control byte, -1 while there is none
  uint32_t ack;    // 1 once an ACK has been seen
  FSK_XT_FN void init() { first = -1; ack = 0u; }
  FSK_XT_FN void byte(uint32_t b) {
    if (first < 0 && (b == kACK || b == kNAK || b == kEOT)) first = (int32_t)b;
    if (b == kACK) ack = 1u;
  }
  // nothing behind this point can change what a sender in `state` does with the reply
  FSK_XT_FN bool settled(uint32_t state) const { return state == FSKHIP_XT_WAIT_FINAL_ACK ? ack != 0u : first >= 0; }
  // 16 bytes at once, little-endian words, bytes [lo, hi) of them (positions 0..15)
  FSK_XT_FN void quad(const uint32_t w[4], uint32_t lo, uint32_t hi) {
    for (uint32_t q = lo; q < hi; q++) byte((w[q >> 2] >> ((q & 3u) * 8u)) & 0xFFu);
  }
};

// the sender's words of one stream
struct Words {
  uint32_t state, sequence, index, n_fragments, retries, sent, retransmitted;
};

struct Step {
  fskhip_xmodem_tx_event ev;
  uint32_t send;      // SEND_*: fragment ev.fragment_index with sequence ev.sequence, or the single byte EOT
  uint32_t touched;   // a sender word changes
  uint32_t drained;   // the reply was taken: the whole ring content leaves
  uint32_t listed;
};

// bytes of fragment `index` of a file of file_len bytes cut into slices of max_payload (createFragments, xmodem.ts:504-514)
FSK_XT_FN uint32_t fragment_len(uint32_t file_len, uint32_t max_payload, uint32_t index) {
  const uint64_t first = (uint64_t)index * max_payload;
  if (first >= file_len) return 0u;
  const uint64_t left = file_len - first;
  return left < max_payload ? (uint32_t)left : max_payload;
}
FSK_XT_FN uint32_t fragment_count(uint32_t file_len, uint32_t max_payload) {
  const uint32_t n = (uint32_t)(((uint64_t)file_len + max_payload - 1u) / max_payload);
  return n ? n : 1u;   // an empty file is ONE empty fragment
}

// One poll of a SELECTED stream (state != IDLE): rules 1-3 of the contract.  `pending`: the processor's tx_pending; F: the find
// over the live ring bytes (looked at only under rule 3).  W is updated in place.
FSK_XT_FN Step step(Words &W, bool abort, bool pending, const Find &F, uint32_t max_retries, uint32_t file_len, uint32_t max_payload) {
  Step R;
  R.send = SEND_NOTHING; R.touched = 0u; R.drained = 0u; R.listed = 0u;
  uint32_t status = FSKHIP_XT_PROGRESS, sent_len = 0u;
  int32_t control = -1;
  if (abort) {   // a timeout: every wait throws, nothing retries (xmodem.ts:391, 409, 444, 617-619)
    status = FSKHIP_XT_ABORTED;
    W.state = FSKHIP_XT_IDLE;
    R.touched = 1u;
  } else if (!pending) {   // (a stream still inside `await modulate()` is not waiting yet)
    R.drained = 1u; R.touched = 1u;
    bool packet = false;
    if (W.state == FSKHIP_XT_WAIT_NAK) {   // waitAndSkipForControl(NAK): an ACK or an EOT is returned and skipped
      control = F.first;
      if (control == (int32_t)kNAK) { packet = true; W.state = FSKHIP_XT_WAIT_ACK; }
    } else if (W.state == FSKHIP_XT_WAIT_ACK) {   // xmodem.ts:137-151 inside withRetry
      control = F.first;
      if (control == (int32_t)kACK) {
        W.retries = 0u;   // (the next withRetry call starts its own counter)
        W.index++;
        W.sequence = (W.sequence % 255u) + 1u;
        if (W.index < W.n_fragments) packet = true;
        else { R.send = SEND_EOT; sent_len = 1u; W.sent++; W.state = FSKHIP_XT_WAIT_FINAL_ACK; }
      } else if (control == (int32_t)kNAK) {
        W.retransmitted++;                    // xmodem.ts:146
        if (++W.retries > max_retries) {      // xmodem.ts:621
          status = FSKHIP_XT_MAX_RETRIES;
          W.state = FSKHIP_XT_IDLE;
        } else {
          W.retransmitted++;                  // onRetry, xmodem.ts:155
          packet = true;
        }
      }
    } else {   // WAIT_FINAL_ACK: waitForACK, the echo of the sender's own EOT and everything else ignored
      if (F.ack) { control = (int32_t)kACK; status = FSKHIP_XT_DONE; W.state = FSKHIP_XT_IDLE; }
    }
    if (packet) {
      R.send = SEND_PACKET;
      sent_len = fragment_len(file_len, max_payload, W.index) + 6u;
      W.sent++;
    }
  }
  R.ev.status = status; R.ev.state_after = W.state; R.ev.control = control; R.ev.sent_len = sent_len;
  R.ev.sequence = W.sequence; R.ev.fragment_index = W.index; R.ev.n_fragments = W.n_fragments; R.ev.retries = W.retries;
  R.listed = (status != FSKHIP_XT_PROGRESS || sent_len != 0u || control != -1) ? 1u : 0u;
  return R;
}

}  // namespace xt
}  // namespace fsk
