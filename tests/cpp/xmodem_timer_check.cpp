// The resident XModem wait timers' rule (webaudio_modem_amd/csrc/fsk_xmodem_timer.h) as a host program, walked together with the
// two transitions it surrounds (fsk_xmodem_recv_step.h with the one-reply scan, fsk_xmodem_tx_step.h): the same text the fire, step
// and arm kernels compile for the device.  One stream at a time: a timed poll here is fire -> step -> (committed: the ring and the
// words move as the commit kernels move them, then arm | stood down: the timer's words go back).  Every sequence below is scripted,
// and the flag and the two words it must give after every poll are written out by hand.  Prints one line per failed expectation
// and exits 1 if there was one.  Built by tests/test_xmodem_timer_cpu.py with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "fsk_xmodem_recv_step.h"
#include "fsk_xmodem_timer.h"
#include "fsk_xmodem_tx_step.h"

using namespace fsk;

static int g_failed = 0, g_checked = 0;
static uint32_t g_table[256];

struct Got { uint32_t flag, listed, status; int32_t control; };

static void expect(const char *what, int step, const xw::Words &T, const Got &G, uint32_t flag, uint32_t waited, uint32_t mark) {
  g_checked++;
  if (G.flag == flag && T.waited == waited && T.mark == mark) return;
  g_failed++;
  std::printf("%s, poll %d: flag %u waited %u mark %u, expected flag %u waited %u mark %u\n", what, step, G.flag, T.waited, T.mark, flag, waited, mark);
}
static void expect_eq(const char *what, long got, long want) {
  g_checked++;
  if (got == want) return;
  g_failed++;
  std::printf("%s: %ld, expected %ld\n", what, got, want);
}

static std::vector<uint8_t> packet(uint32_t seq, const std::vector<uint8_t> &payload) {
  std::vector<uint8_t> p = {(uint8_t)xm::kSOH, (uint8_t)seq, (uint8_t)(255u - seq), (uint8_t)payload.size()};
  uint32_t crc = 0xFFFFu;
  for (uint8_t b : payload) { p.push_back(b); crc = xm::crc_step(g_table, crc, b); }
  p.push_back((uint8_t)(crc >> 8)); p.push_back((uint8_t)(crc & 0xFFu));
  return p;
}

struct Recv {
  xr::Words W{FSKHIP_XR_SEND_NAK, 1u, 0u, 0u, 0u, 0u, 0u};
  std::vector<uint8_t> ring;
  bool pending = true;   // start() has sent the NAK
  xw::Words T{0u, 0u};
  uint32_t timeout = 1000u, max_retries = 2u;
  void feed(const std::vector<uint8_t> &b, size_t from, size_t to) { ring.insert(ring.end(), b.begin() + (long)from, b.begin() + (long)to); }
  Got poll(uint32_t elapsed, bool commit = true, bool abort = false) {
    const xw::Words before = T;
    const uint32_t held = (uint32_t)ring.size();
    const uint32_t flag = xw::fire(T, pending, W.state == FSKHIP_XR_SEND_NAK || W.state == FSKHIP_XR_SEND_ACK, elapsed, timeout);
    const bool was_waiting = !pending, look = !abort && !pending;
    const uint32_t n = look ? held : 0u;
    xm::Scan sc;
    sc.init(look ? W.expected : 1u);
    for (uint32_t pos = 0; pos < n && !sc.owes_reply(); pos++) sc.byte<false>(g_table, ring[pos], pos, nullptr, 0);
    xr::Words after = W;
    const xr::Step R = xr::step(after, abort, pending, look && flag != 0u, xr::found_of(sc), n, max_retries, 4096u);
    if (!commit) { T = before; return Got{flag, R.listed, R.ev.status, R.ev.control}; }   // stood down: nothing moves
    W = after;
    ring.erase(ring.begin(), ring.begin() + (long)(R.removed <= held ? R.removed : held));
    if (R.ev.control != -1) pending = true;
    xw::arm_recv(T, was_waiting, R.ev.status, R.ev.state_after, R.ev.control, was_waiting ? held : 0u, was_waiting ? (uint32_t)ring.size() : 0u);
    return Got{flag, R.listed, R.ev.status, R.ev.control};
  }
};

struct Send {
  xt::Words W{FSKHIP_XT_WAIT_NAK, 1u, 0u, 1u, 0u, 0u, 0u};   // one file of 10 bytes, one fragment
  std::vector<uint8_t> ring;
  bool pending = false;
  xw::Words T{0u, 0u};
  uint32_t timeout = 1000u;
  Got poll(uint32_t elapsed, bool commit = true, bool abort = false) {
    const xw::Words before = T;
    const uint32_t flag = xw::fire(T, pending, false, elapsed, timeout);
    const bool was_waiting = !pending, ab = abort || flag != 0u, look = !ab && !pending;
    xt::Find F;
    F.init();
    if (look)
      for (size_t i = 0; i < ring.size() && !F.settled(W.state); i++) F.byte(ring[i]);
    xt::Words after = W;
    const xt::Step R = xt::step(after, ab, pending, F, 2u, 10u, 16u);
    if (!commit) { T = before; return Got{flag, R.listed, R.ev.status, R.ev.control}; }
    W = after;
    if (R.drained) ring.clear();
    if (R.send != xt::SEND_NOTHING) pending = true;
    xw::arm_tx(T, was_waiting, R.ev.status, R.ev.state_after, R.ev.control, R.ev.sent_len);
    return Got{flag, R.listed, R.ev.status, R.ev.control};
  }
};

// a stream pending for several polls, then waiting: the time spent pending does not count
static void pending_time_does_not_count() {
  const char *w = "pending";
  Recv R;
  for (int i = 0; i < 4; i++) expect(w, i, R.T, R.poll(400u), 0u, 0u, 4u);   // 1600 samples inside `await sendControl()`
  R.pending = false;
  expect(w, 4, R.T, R.poll(400u), 0u, 0u, 0u);      // the wait begins at this poll
  expect_eq("pending: SEND_NAK became WAIT_BLOCK", R.W.state, FSKHIP_XR_WAIT_BLOCK);
  expect(w, 5, R.T, R.poll(400u), 0u, 400u, 0u);
  expect(w, 6, R.T, R.poll(400u), 0u, 800u, 0u);
  const Got G = R.poll(400u);                       // 1200 >= 1000: the timer fires, the poll NAKs, the timer is re-armed
  expect(w, 7, R.T, G, 1u, 0u, 0u);
  expect_eq("pending: the timeout's control byte", G.control, (long)xr::kNAK);
  expect_eq("pending: retries", R.W.retries, 1);
  expect(w, 8, R.T, R.poll(400u), 0u, 0u, 4u);      // the NAK is being modulated
  R.pending = false;
  expect(w, 9, R.T, R.poll(5000u), 0u, 0u, 0u);     // however long the modulation took
  // a receiver whose pending modulation no timed poll saw: the SEND_* state alone begins the wait
  Recv Q;
  Q.pending = false; Q.T = xw::Words{777u, 2u};
  expect("pending (unseen)", 0, Q.T, Q.poll(100u), 0u, 0u, 0u);
}

// elapsed sums that cross timeout_samples exactly, one short of it, and at saturation
static void crossing() {
  const char *w = "crossing";
  Recv R;
  R.pending = false; R.W.state = FSKHIP_XR_WAIT_BLOCK;
  expect(w, 0, R.T, R.poll(500u), 0u, 500u, 0u);
  expect(w, 1, R.T, R.poll(499u), 0u, 999u, 0u);    // one short
  const Got G = R.poll(1u);                         // exactly
  expect(w, 2, R.T, G, 1u, 0u, 0u);
  expect_eq("crossing: listed", G.listed, 1);
  xw::Words T{0xFFFFFFF0u, 0u};
  expect_eq("saturation: below", xw::fire(T, false, false, 0xEu, 0xFFFFFFFFu), 0);
  expect_eq("saturation: waited below", T.waited, 0xFFFFFFFEu);
  expect_eq("saturation: at", xw::fire(T, false, false, 0x20u, 0xFFFFFFFFu), 1);
  expect_eq("saturation: waited at", T.waited, 0xFFFFFFFFu);
  expect_eq("saturation: stays", xw::fire(T, false, false, 0xFFFFFFFFu, 0xFFFFFFFFu), 1);
  expect_eq("saturation: waited stays", T.waited, 0xFFFFFFFFu);
  expect_eq("sat_add", xw::sat_add(0x80000000u, 0x80000000u), 0xFFFFFFFFu);
}

// a noise byte ends a waitForByte and the loop arms a new one
static void noise() {
  const char *w = "noise";
  Recv R;
  R.pending = false; R.W.state = FSKHIP_XR_WAIT_BLOCK;
  expect(w, 0, R.T, R.poll(600u), 0u, 600u, 0u);
  R.ring = {0x55};
  const Got G = R.poll(100u);
  expect(w, 1, R.T, G, 0u, 0u, 0u);
  expect_eq("noise: not listed", G.listed, 0);
  expect_eq("noise: the byte left", (long)R.ring.size(), 0);
  expect(w, 2, R.T, R.poll(100u), 0u, 100u, 0u);
}

// stage 0 -> 1 -> 2 re-arms; payload bytes trickling in inside stage 2 do not; an accepted packet and a duplicate re-arm
static void stages() {
  const char *w = "stages";
  Recv R;
  R.pending = false; R.W.state = FSKHIP_XR_WAIT_BLOCK;
  const std::vector<uint8_t> P = packet(1u, {10, 20, 30, 40, 50, 60});   // 12 bytes
  expect(w, 0, R.T, R.poll(300u), 0u, 300u, 0u);
  R.feed(P, 0, 1);                                   // SOH
  expect(w, 1, R.T, R.poll(100u), 0u, 0u, 1u);       // stage 0 -> 1
  expect(w, 2, R.T, R.poll(100u), 0u, 100u, 1u);
  R.feed(P, 1, 3);                                   // seq, ~seq: still the header wait
  expect(w, 3, R.T, R.poll(100u), 0u, 200u, 1u);
  R.feed(P, 3, 4);                                   // len: the header is whole
  expect(w, 4, R.T, R.poll(100u), 0u, 0u, 2u);       // stage 1 -> 2
  R.feed(P, 4, 6);
  expect(w, 5, R.T, R.poll(100u), 0u, 100u, 2u);     // payload bytes trickle: one wait
  R.feed(P, 6, 11);
  expect(w, 6, R.T, R.poll(100u), 0u, 200u, 2u);
  expect_eq("stages: the packet waits in the ring", (long)R.ring.size(), 11);
  R.feed(P, 11, 12);
  Got G = R.poll(100u);                              // accepted: ACK, re-armed
  expect(w, 7, R.T, G, 0u, 0u, 0u);
  expect_eq("stages: accepted", G.control, (long)xr::kACK);
  expect_eq("stages: file_len", R.W.file_len, 6);
  expect(w, 8, R.T, R.poll(100u), 0u, 0u, 4u);       // ACK being modulated
  R.pending = false;
  expect(w, 9, R.T, R.poll(200u), 0u, 0u, 0u);
  expect(w, 10, R.T, R.poll(200u), 0u, 200u, 0u);
  expect(w, 11, R.T, R.poll(200u), 0u, 400u, 0u);
  R.feed(P, 0, 12);                                  // the same packet again: a duplicate
  G = R.poll(200u);
  expect(w, 12, R.T, G, 0u, 0u, 0u);
  expect_eq("stages: duplicate", R.W.dropped, 1);
  expect_eq("stages: duplicate's ACK", G.control, (long)xr::kACK);
  // a timeout inside stage 2 clears the ring and NAKs
  R.pending = false; R.T = xw::Words{0u, 0u}; R.W.state = FSKHIP_XR_WAIT_BLOCK;
  const std::vector<uint8_t> P2 = packet(2u, {1, 2, 3});
  R.feed(P2, 0, 5);
  expect(w, 13, R.T, R.poll(10u), 0u, 0u, 2u);       // stage 0 -> 2 at once
  expect(w, 14, R.T, R.poll(989u), 0u, 989u, 2u);
  G = R.poll(11u);
  expect(w, 15, R.T, G, 1u, 0u, 0u);
  expect_eq("stages: timeout NAK", G.control, (long)xr::kNAK);
  expect_eq("stages: ring cleared", (long)R.ring.size(), 0);
}

// the sender: one waitAndSkipForControl keeps one timer, each turn of the WAIT_ACK loop arms its own
static void sender() {
  const char *w = "sender";
  Send S;
  expect(w, 0, S.T, S.poll(300u), 0u, 300u, 0u);
  S.ring = {(uint8_t)xt::kACK};                      // returned and skipped in WAIT_NAK: the timer runs on
  Got G = S.poll(300u);
  expect(w, 1, S.T, G, 0u, 600u, 0u);
  expect_eq("sender: skipped ACK listed", G.listed, 1);
  S.ring = {(uint8_t)xt::kNAK};
  G = S.poll(300u);                                  // 900 < 1000: the NAK starts fragment 0
  expect(w, 2, S.T, G, 0u, 0u, 0u);
  expect_eq("sender: state", S.W.state, FSKHIP_XT_WAIT_ACK);
  for (int i = 3; i < 6; i++) expect(w, i, S.T, S.poll(300u), 0u, 0u, 4u);   // `await modulate()`
  S.pending = false;
  expect(w, 6, S.T, S.poll(300u), 0u, 0u, 0u);
  expect(w, 7, S.T, S.poll(300u), 0u, 300u, 0u);
  S.ring = {'x', 'y'};                               // no control bytes: waitForControlByte goes on waiting
  G = S.poll(300u);
  expect(w, 8, S.T, G, 0u, 600u, 0u);
  expect_eq("sender: drained", (long)S.ring.size(), 0);
  expect_eq("sender: not listed", G.listed, 0);
  S.ring = {(uint8_t)xt::kEOT};                      // an EOT in WAIT_ACK: the loop turns, a new timer
  G = S.poll(300u);
  expect(w, 9, S.T, G, 0u, 0u, 0u);
  expect_eq("sender: EOT returned", G.control, (long)xt::kEOT);
  expect(w, 10, S.T, S.poll(999u), 0u, 999u, 0u);
  G = S.poll(1u);                                    // the timer fires: 'Operation aborted', nothing retried
  expect(w, 11, S.T, G, 1u, 0u, 0u);
  expect_eq("sender: aborted", G.status, FSKHIP_XT_ABORTED);
  expect_eq("sender: idle", S.W.state, FSKHIP_XT_IDLE);
  // a caller's abort of a pending stream ends it too, and the timer is a fresh one
  Send A;
  A.W.state = FSKHIP_XT_WAIT_ACK; A.pending = true; A.T = xw::Words{0u, 0u};
  expect("sender (abort)", 0, A.T, A.poll(100u), 0u, 0u, 4u);
  expect("sender (abort)", 1, A.T, A.poll(100u, true, true), 0u, 0u, 0u);
  expect_eq("sender (abort): idle", A.W.state, FSKHIP_XT_IDLE);
}

// a stood-down (overflow) poll leaves every word as it was
static void stood_down() {
  Recv R;
  R.pending = false; R.W.state = FSKHIP_XR_WAIT_BLOCK; R.T = xw::Words{500u, 1u};
  R.ring = {(uint8_t)xm::kSOH, 1u};
  Got G = R.poll(700u, false);
  expect("stood down", 0, R.T, G, 1u, 500u, 1u);     // the flag was raised and handed on, and nothing came of it
  expect_eq("stood down: state", R.W.state, FSKHIP_XR_WAIT_BLOCK);
  expect_eq("stood down: ring", (long)R.ring.size(), 2);
  Recv P;                                            // a pending stream: the was-pending bit is undone as well
  expect("stood down (pending)", 0, P.T, P.poll(700u, false), 0u, 0u, 0u);
  Send S;
  S.T = xw::Words{990u, 0u};
  expect("stood down (sender)", 0, S.T, S.poll(700u, false), 1u, 990u, 0u);
  expect_eq("stood down (sender): state", S.W.state, FSKHIP_XT_WAIT_NAK);
  // the committed poll that follows does what the first would have done
  G = R.poll(700u);
  expect("stood down", 1, R.T, G, 1u, 0u, 0u);
  expect_eq("stood down: NAK after all", G.control, (long)xr::kNAK);
}

static void marks() {
  expect_eq("valid_mark 0", xw::valid_mark(0u), 1);
  expect_eq("valid_mark 6", xw::valid_mark(6u), 1);
  expect_eq("valid_mark 3", xw::valid_mark(3u), 0);
  expect_eq("valid_mark 8", xw::valid_mark(8u), 0);
  expect_eq("recv_stage", (long)(xw::recv_stage(0u) * 100u + xw::recv_stage(1u) * 10u + xw::recv_stage(3u) * 10u + xw::recv_stage(4u)), 22);
}

int main() {
  for (uint32_t i = 0; i < 256u; i++) g_table[i] = xm::crc_table_entry(i);
  pending_time_does_not_count();
  crossing();
  noise();
  stages();
  sender();
  stood_down();
  marks();
  std::printf("%d expectations, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
