// fsk_xmodem_recv_step.h -- XModemTransport's receiveData() as one transition per poll, defined once: the resident file
// receiver's step kernel (fsk_xmodem_recv.hip) and a host program (tests/cpp/xmodem_recv_step_check.cpp) include the same text.
// What it restates: receiveAllPackets and receiveAndProcessPacket, src/transports/xmodem/xmodem.ts:233-320 -- what the loop does
// with the FIRST step of the receive grammar that owes a reply (fsk_xmodem_scan.h, one-reply mode), or with a wait whose timer
// fired -- pinned to the real class by tests/golden/golden_xmodem_recv.npz.  The contract is in include/fskhip_next.h.
// Plain C++ as well as HIP (FSK_XR_FN is plain `inline` without a device compiler).  Not part of the ABI.
#pragma once
#include <stdint.h>

#include "../../include/fskhip_next.h"
#include "fsk_xmodem_scan.h"

#if defined(__HIPCC__)
#define FSK_XR_FN __device__ __forceinline__
#else
#define FSK_XR_FN inline
#endif

namespace fsk {
namespace xr {

constexpr uint32_t kACK = 0x06, kNAK = 0x15;   // types.ts:29-34

// what the one-reply walk over the live ring bytes found (xm::Scan's fields, copied out so that host code can fill it too)
struct Found {
  uint32_t status;      // FSKHIP_XM_* of the walk
  uint32_t packets, dropped, consumed, start, seq, len, expected;
  int32_t err_seq, err_len, crc_rx, crc_calc;
  uint32_t inside;      // the walk ended inside a packet
};

// the receiver's words of one stream
struct Words {
  uint32_t state, expected, retries, file_len, packets, dropped, sent;
};

struct Step {
  fskhip_xmodem_recv_event ev;
  uint32_t touched;   // a receiver word or the ring changes
  uint32_t listed;
  uint32_t removed;   // bytes that leave the ring's front
  uint32_t span;      // where the accepted payload starts in L (ev.accepted_len bytes; appended at ev.file_len - ev.accepted_len)
  uint32_t appended;  // 1: an accepted payload is appended (it may be empty)
};

FSK_XR_FN bool is_error(uint32_t status) {
  return status == FSKHIP_XM_INVALID_SEQUENCE || status == FSKHIP_XM_INVALID_CRC || status == FSKHIP_XM_UNEXPECTED_SEQUENCE;
}

// One poll of a SELECTED stream (state != IDLE): rules 1-3 of the contract.  `pending`: the processor's tx_pending; F: the
// one-reply walk over the n live ring bytes (looked at only under rule 3).  W is updated in place.
FSK_XR_FN Step step(Words &W, bool abort, bool pending, bool timeout, const Found &F, uint32_t n, uint32_t max_retries, uint32_t file_capacity) {
  Step R;
  R.touched = 0u; R.listed = 0u; R.removed = 0u; R.span = 0u; R.appended = 0u;
  uint32_t status = FSKHIP_XR_PROGRESS, step_status = FSKHIP_XM_NEED_MORE, accepted_len = 0u;
  int32_t control = -1, seq = -1, len = -1, crc_rx = -1, crc_calc = -1;
  if (abort) {   // checkAbort (xmodem.ts:235): 'Operation aborted'
    status = FSKHIP_XR_ABORTED;
    W.state = FSKHIP_XR_IDLE;
    R.touched = 1u;
  } else if (!pending) {   // (a stream still inside `await sendControl()` reads nothing and runs no timer)
    R.touched = 1u;
    if (W.state != FSKHIP_XR_WAIT_BLOCK) W.state = FSKHIP_XR_WAIT_BLOCK;   // the control byte has gone out (xmodem.ts:230, 306)
    step_status = F.status;
    bool failed = false;   // the catch of receiveAllPackets (xmodem.ts:253-262)
    if (F.status == FSKHIP_XM_EOT) {   // xmodem.ts:240-243
      R.removed = F.consumed;
      control = (int32_t)kACK;
      status = FSKHIP_XR_DONE;
      W.state = FSKHIP_XR_IDLE;
    } else if (is_error(F.status)) {
      W.packets += F.packets; W.dropped += F.dropped;
      seq = F.err_seq; len = F.err_len; crc_rx = F.crc_rx; crc_calc = F.crc_calc;
      failed = true;
    } else if (F.packets) {   // accepted (xmodem.ts:293-307)
      seq = (int32_t)F.seq; len = (int32_t)F.len;
      if (F.len > file_capacity - W.file_len) {   // the resident store's own limit: the packet stays where it is
        status = FSKHIP_XR_FILE_FULL;
        W.state = FSKHIP_XR_IDLE;
        R.removed = F.start;
      } else {
        R.appended = 1u; R.span = F.start + 4u; accepted_len = F.len;
        W.file_len += F.len;
        W.expected = F.expected;
        W.retries = 0u;
        W.packets++;
        R.removed = F.consumed;
        control = (int32_t)kACK;
        W.state = FSKHIP_XR_SEND_ACK;
      }
    } else if (F.dropped) {   // a duplicate (xmodem.ts:309-314): ACKed, retries untouched
      seq = (int32_t)F.seq; len = (int32_t)F.len;
      W.dropped++;
      R.removed = F.consumed;
      control = (int32_t)kACK;
    } else {   // no step that owes a reply: noise leaves, an incomplete packet waits
      R.removed = F.inside ? F.start : F.consumed;
      if (timeout) failed = true;   // the wait's timer fired: caught like any error
    }
    if (failed) {
      R.removed = n;   // receive.buffer = [] -- everything that arrived is in it
      if (++W.retries > max_retries) {   // 'Receive failed after max retries: ...'
        status = FSKHIP_XR_MAX_RETRIES;
        W.state = FSKHIP_XR_IDLE;
      } else {
        control = (int32_t)kNAK;
      }
    }
    if (control != -1) W.sent++;
  }
  R.ev.status = status; R.ev.state_after = W.state; R.ev.control = control; R.ev.step = step_status;
  R.ev.seq = seq; R.ev.len = len; R.ev.accepted_len = accepted_len;
  R.ev.file_len = W.file_len; R.ev.expected = W.expected; R.ev.retries = W.retries;
  R.ev.crc_rx = crc_rx; R.ev.crc_calc = crc_calc;
  R.listed = (status != FSKHIP_XR_PROGRESS || control != -1) ? 1u : 0u;
  return R;
}

// Found of a finished one-reply walk
FSK_XR_FN Found found_of(const xm::Scan &sc) {
  Found F;
  F.status = sc.status; F.packets = sc.packets; F.dropped = sc.dropped; F.consumed = sc.consumed; F.start = sc.start;
  F.seq = sc.seq; F.len = sc.len; F.expected = sc.expected;
  F.err_seq = sc.err_seq; F.err_len = sc.err_len; F.crc_rx = sc.crc_rx; F.crc_calc = sc.crc_calc;
  F.inside = sc.inside_packet() ? 1u : 0u;
  return F;
}

}  // namespace xr
}  // namespace fsk
