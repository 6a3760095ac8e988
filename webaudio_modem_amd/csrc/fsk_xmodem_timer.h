// fsk_xmodem_timer.h -- the wait timers of XModemTransport's sendData() / receiveData() in the engine's sample clock, defined once:
// the fire and arm kernels (fsk_xmodem_timer.hip) and a host program (tests/cpp/xmodem_timer_check.cpp) include the same text.
// What it restates: where the reference arms a `timeoutMs` timer -- each waitForByte / waitForBytes call of the receiver
// (src/transports/xmodem/xmodem.ts:238, 267, 279, 311) and each waitForControlByte / waitAndSkipForControl / waitForACK of the
// sender (xmodem.ts:138, 111, 174) -- and that no timer runs inside `await sendControl()` / `await modulate()`.  A timed poll is
// fire -> the existing poll (fsk_xmodem_recv_step.h / fsk_xmodem_tx_step.h, unchanged) -> arm; the contract is in
// include/fskhip_next.h.  The timers are QUANTISED TO THE POLLS: time passes only as the `elapsed` of a timed poll, so a wait ends
// at the first poll at or after its deadline, never between two polls.  They are meant for one poll per quantum.
// Plain C++ as well as HIP (FSK_XW_FN is plain `inline` without a device compiler).  Not part of the ABI.
#pragma once
#include <stdint.h>

#include "../../include/fskhip_next.h"

#if defined(__HIPCC__)
#define FSK_XW_FN __host__ __device__ __forceinline__
#else
#define FSK_XW_FN inline
#endif

namespace fsk {
namespace xw {

constexpr uint32_t kEOT = 0x04;   // types.ts:29-34
// `mark`: the stage the timer was armed for (bits 0-1: 0..2, always 0 for a sender) and the was-pending bit
constexpr uint32_t kStageMask = 3u, kWasPending = 4u;
// what the fire pass found a stream to be, kept in scratch for the arm pass
enum : uint32_t { NOT_SELECTED = 0, PENDING = 1, WAITING = 2 };

// the two words of one stream
struct Words {
  uint32_t waited;   // engine samples this wait has lasted, saturating
  uint32_t mark;
};

FSK_XW_FN uint32_t sat_add(uint32_t a, uint32_t b) {
  const uint32_t s = a + b;
  return s < a ? 0xFFFFFFFFu : s;
}

FSK_XW_FN bool valid_mark(uint32_t mark) { return (mark & ~(kStageMask | kWasPending)) == 0u && (mark & kStageMask) <= 2u; }

// FIRE, before the poll, for a stream the poll will select (mask set, state not IDLE).  pending: the processor's tx_pending;
// begins: the receiver's state is SEND_NAK / SEND_ACK, so its wait begins at this poll (always false for a sender).
// Returns the flag: the receiver's timeout[s], or what is OR-ed into the sender's abort[s].
FSK_XW_FN uint32_t fire(Words &T, bool pending, bool begins, uint32_t elapsed, uint32_t timeout_samples) {
  if (pending) {   // inside `await sendControl()` / `await modulate()`: no timer runs, and the time spent there never counts
    T.mark |= kWasPending;
    return 0u;
  }
  if ((T.mark & kWasPending) || begins) {   // the wait begins at this poll
    T.waited = 0u;
    T.mark = 0u;
  } else {
    T.waited = sat_add(T.waited, elapsed);
  }
  return T.waited >= timeout_samples ? 1u : 0u;
}

// the receiver's stage from the live bytes a poll left in the ring.  A poll that found no reply-owing step leaves either nothing
// or an incomplete packet with its SOH at the ring's front (noise leaves), so the count alone tells them apart:
//   0  no live byte                                 waitForByte, xmodem.ts:238
//   1  an SOH and fewer than 4 live bytes           waitForBytes(3), xmodem.ts:267
//   2  4 or more live bytes, the walk NEED_MORE     waitForBytes of the payload and the CRC, xmodem.ts:279, 311
FSK_XW_FN uint32_t recv_stage(uint32_t live) { return live == 0u ? 0u : live < 4u ? 1u : 2u; }

// ARM, after a COMMITTED poll, for a stream that fire found PENDING or WAITING.  A poll that stood down is undone instead: both
// words go back to what they were before fire.
// The receiver.  status / state_after / control: the poll's event of the stream (written for every selected stream, listed or
// not); held: the ring's live bytes before the poll (what fire saved); live: after it.
FSK_XW_FN void arm_recv(Words &T, bool was_waiting, uint32_t status, uint32_t state_after, int32_t control, uint32_t held, uint32_t live) {
  if (state_after == FSKHIP_XR_IDLE) { T.waited = 0u; T.mark = 0u; return; }   // the transfer ended
  if (!was_waiting) return;
  const bool listed = status != FSKHIP_XR_PROGRESS || control != -1;   // something was transmitted
  const uint32_t stage = recv_stage(live);
  // not listed: no reply-owing step was found, so bytes that left were noise -- it ends a waitForByte and the loop arms a new
  // one (xmodem.ts:247-250); a higher stage is the next wait of the packet.  Payload bytes trickling in inside stage 2 are one wait.
  if (listed || live < held || stage > (T.mark & kStageMask)) T.waited = 0u;
  T.mark = (T.mark & ~kStageMask) | stage;
}

// The sender.  One waitAndSkipForControl / waitForACK keeps one timer (xmodem.ts:111, 174): a skipped ACK or EOT in WAIT_NAK and
// anything in WAIT_FINAL_ACK leave it running.  Each turn of the WAIT_ACK loop arms its own (xmodem.ts:137-151): an EOT returned
// there re-arms it, bytes that are no control bytes do not (waitForControlByte goes on waiting for them).
FSK_XW_FN void arm_tx(Words &T, bool was_waiting, uint32_t status, uint32_t state_after, int32_t control, uint32_t sent_len) {
  if (state_after == FSKHIP_XT_IDLE) { T.waited = 0u; T.mark = 0u; return; }   // the transfer ended
  if (!was_waiting) return;
  if (sent_len != 0u || status != FSKHIP_XT_PROGRESS) T.waited = 0u;
  else if (state_after == FSKHIP_XT_WAIT_ACK && control == (int32_t)kEOT) T.waited = 0u;
}

}  // namespace xw
}  // namespace fsk
