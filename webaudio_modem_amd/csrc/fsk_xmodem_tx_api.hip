// fsk_xmodem_tx_api.hip -- C ABI of the resident XModem sender (include/fskhip_next.h: fskhip_xmodem_tx_*): a handle over an
// FSKProcessor batch that keeps every stream's file in one packed store on the device together with the send state and the two
// counters, and polls the RX rings for the control bytes the waits of sendData() wait for (fsk_xmodem_tx.hip).  A poll that finds
// one builds the next packet on the device and starts its modulation; the timers and the decision to abort stay with the host
// (DESIGN.md section 8).
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "fsk_host.h"
#include "fsk_launch.h"
#include "fsk_proc.h"
#include "fsk_xmodem_handles.h"
#include "fsk_xmodem_tx_step.h"

using namespace fsk;

namespace {

const char *const kStateNames[] = {"IDLE", "SENDING_WAIT_NAK", "SENDING_WAIT_ACK", "SENDING_WAIT_FINAL_ACK"};   // xmodem.ts:22-32

// what both forms of the poll refuse before they touch the device, in the header's order
int poll_refusal(const char *fn, const fskhip_xmodem_tx *t, const void *totals, const char *totals_name, const void *streams, const void *events,
                 uint32_t cap_streams) {
  if (!totals) return fail(FSKHIP_E_INVALID, "%s: null %s", fn, totals_name);
  if (cap_streams && (!streams || !events)) return fail(FSKHIP_E_INVALID, "%s: null streams or events with cap_streams %u", fn, cap_streams);
  if (!t) return fail(FSKHIP_E_INVALID, "null sender");
  return FSKHIP_OK;
}

// the store holds `live` bytes of files that stay and is about to take `incoming` more at its end: where they do not fit behind
// `used`, the files that stay move to the front of a new, larger store
int make_room(fskhip_xmodem_tx *t, const std::vector<uint8_t> &stays, uint64_t live, uint64_t incoming) {
  if (t->store_used + incoming <= t->store_cap) return FSKHIP_OK;
  const size_t S = t->p->S;
  uint64_t cap = 2u * (live + incoming);
  if (cap < 4096u) cap = 4096u;
  if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
  uint8_t *fresh = nullptr;
  int rc = dev_alloc(fresh, (size_t)cap);
  if (rc != FSKHIP_OK) return rc;
  std::vector<uint32_t> new_off(S, 0u);
  uint32_t at = 0u;
  for (size_t s = 0; s < S; s++)
    if (stays[s]) { new_off[s] = at; at += t->h_len[s]; }
  if (live) {
    HIP_TRY_AS(hipMemcpy(t->d_new_off, new_off.data(), sizeof(uint32_t) * S, hipMemcpyHostToDevice), "hipMemcpy", false, (void)hipFree(fresh));
    HIP_TRY_AS(hipMemcpy(t->d_keep, stays.data(), S, hipMemcpyHostToDevice), "hipMemcpy", false, (void)hipFree(fresh));
    HIP_TRY_AS(launch_xmodem_tx_repack(t->d_store, t->X.file_off, t->d_new_off, t->X.file_len, t->d_keep, t->p->S, fresh, nullptr), "repack", false,
               (void)hipFree(fresh));
    HIP_TRY_AS(hipDeviceSynchronize(), "hipDeviceSynchronize", false, (void)hipFree(fresh));
  }
  if (t->d_store) (void)hipFree(t->d_store);
  t->d_store = fresh; t->store_cap = (size_t)cap; t->store_used = at;
  t->X.store = fresh;
  for (size_t s = 0; s < S; s++)
    if (stays[s]) t->h_off[s] = new_off[s];
  return FSKHIP_OK;
}

}  // namespace

extern "C" {

int fskhip_xmodem_tx_destroy(fskhip_xmodem_tx *t) {
  if (!t) return FSKHIP_OK;
  xmodem_timers_orphan(t);
  (void)hipSetDevice(t->device);
  (void)hipDeviceSynchronize();
  void *bufs[] = {t->X.state, t->X.sequence, t->X.index, t->X.n_fragments, t->X.retries, t->X.sent, t->X.retransmitted, t->X.file_off, t->X.file_len,
                  t->W.ev, t->W.flags, t->W.pairs, t->W.slab, t->W.tx_lens, t->W.tx_mask, t->d_totals, t->d_store, t->d_new_off, t->d_keep,
                  t->d_mask, t->d_abort, t->d_streams, t->d_events};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  delete t;
  return FSKHIP_OK;
}

int fskhip_xmodem_tx_create(fskhip_processor *p, uint32_t max_payload_size, uint32_t max_retries, fskhip_xmodem_tx **out) {
  if (!p || !out) return fail(FSKHIP_E_INVALID, "fskhip_xmodem_tx_create: null argument");
  if (max_payload_size < 1u || max_payload_size > 255u)
    return fail(FSKHIP_E_INVALID, "fskhip_xmodem_tx_create: max_payload_size %u is not in 1..255", max_payload_size);
  fskhip_xmodem_tx *t = new (std::nothrow) fskhip_xmodem_tx();
  if (!t) return fail(FSKHIP_E_NOMEM, "out of host memory");
  t->p = p;
  t->device = p->device;
  const size_t S = p->S;
  t->X.max_payload = max_payload_size;
  t->X.max_retries = max_retries;
  t->W.slab_pitch = (max_payload_size + 6u + 15u) & ~15u;
  t->h_off.assign(S, 0u); t->h_len.assign(S, 0u); t->h_has.assign(S, 0);
  hipError_t herr = hipSetDevice(p->device);
  if (herr != hipSuccess) { delete t; return fail(FSKHIP_E_HIP, "hipSetDevice: %s", hipGetErrorString(herr)); }
  int rc = FSKHIP_OK;
#define TX_TRY(expr)                  \
  do {                                \
    if (rc == FSKHIP_OK) rc = (expr); \
  } while (0)
  uint32_t **words[] = {&t->X.state, &t->X.sequence, &t->X.index, &t->X.n_fragments, &t->X.retries, &t->X.sent, &t->X.retransmitted, &t->X.file_off,
                        &t->X.file_len, &t->W.flags, &t->W.tx_lens, &t->d_new_off};
  for (uint32_t **w : words) TX_TRY(dev_alloc(*w, S));
  TX_TRY(dev_alloc(t->W.ev, S)); TX_TRY(dev_alloc(t->W.pairs, xmodem_tx_pair_words(p->S))); TX_TRY(dev_alloc(t->d_totals, 4));
  TX_TRY(dev_alloc(t->W.slab, S * t->W.slab_pitch)); TX_TRY(dev_alloc(t->W.tx_mask, S)); TX_TRY(dev_alloc(t->d_keep, S));
  TX_TRY(dev_alloc(t->d_mask, S)); TX_TRY(dev_alloc(t->d_abort, S));
  if (rc == FSKHIP_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipDeviceSynchronize failed");
  for (uint32_t **w : words) TX_TRY(fill_words(*w, S, w == &t->X.sequence ? 1u : 0u));
  if (rc == FSKHIP_OK && S && hipMemset(t->W.slab, 0, S * t->W.slab_pitch) != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipMemset failed");
  TX_TRY(processor_grow_payload(p, max_payload_size + 6u));   // no poll ever needs to allocate
  if (rc == FSKHIP_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipDeviceSynchronize failed");
#undef TX_TRY
  if (rc != FSKHIP_OK) {
    const std::string keep = fskhip_last_error();
    fskhip_xmodem_tx_destroy(t);
    return fail(rc, "%s", keep.c_str());
  }
  *out = t;
  return FSKHIP_OK;
}

int fskhip_xmodem_tx_send_host(fskhip_xmodem_tx *t, const uint8_t *mask, const uint64_t *offsets, const uint8_t *data) {
  static const char fn[] = "fskhip_xmodem_tx_send_host";
  if (!offsets) return fail(FSKHIP_E_INVALID, "%s: null offsets", fn);
  if (!t) return fail(FSKHIP_E_INVALID, "null sender");
  fskhip_processor *p = t->p;
  const size_t S = p->S;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> state, sequence, index, n_fragments, retries;
  int rc;
  if ((rc = get_words(state, t->X.state, S)) != FSKHIP_OK) return rc;
  uint64_t incoming = 0u, live = 0u;
  std::vector<uint8_t> stays(S, 0);
  for (size_t s = 0; s < S; s++) {
    if (mask && !mask[s]) {
      if (t->h_has[s] && t->h_len[s]) { stays[s] = 1; live += t->h_len[s]; }
      continue;
    }
    if (offsets[s] > offsets[s + 1]) return fail(FSKHIP_E_INVALID, "%s: offsets[%zu] exceeds offsets[%zu]", fn, s, s + 1);
    if (offsets[s + 1] > offsets[s] && !data) return fail(FSKHIP_E_INVALID, "%s: null data", fn);
    if (state[s] != FSKHIP_XT_IDLE)   // ensureIdle (xmodem.ts:571-575)
      return fail(FSKHIP_E_BUSY, "Transport busy: sendData cannot start while in %s state (stream %zu)", kStateNames[state[s] & 3u], s);
    incoming += offsets[s + 1] - offsets[s];
  }
  if (live + incoming > 0xFFFFFFFFull)
    return fail(FSKHIP_E_UNSUPPORTED, "%s: the files would take %llu bytes, the store's offsets are 32-bit", fn, (unsigned long long)(live + incoming));
  t->used = true;
  if ((rc = make_room(t, stays, live, incoming)) != FSKHIP_OK) return rc;
  if ((rc = get_words(sequence, t->X.sequence, S)) != FSKHIP_OK || (rc = get_words(index, t->X.index, S)) != FSKHIP_OK ||
      (rc = get_words(n_fragments, t->X.n_fragments, S)) != FSKHIP_OK || (rc = get_words(retries, t->X.retries, S)) != FSKHIP_OK)
    return rc;
  std::vector<uint8_t> packed;
  packed.reserve((size_t)incoming);
  size_t at = t->store_used;
  for (size_t s = 0; s < S; s++) {
    if (mask && !mask[s]) continue;
    const uint32_t len = (uint32_t)(offsets[s + 1] - offsets[s]);
    if (len) packed.insert(packed.end(), data + offsets[s], data + offsets[s + 1]);
    t->h_off[s] = (uint32_t)at; t->h_len[s] = len; t->h_has[s] = 1;
    at += len;
    // initializeSend (xmodem.ts:103-107)
    state[s] = FSKHIP_XT_WAIT_NAK; sequence[s] = 1u; index[s] = 0u; retries[s] = 0u;
    n_fragments[s] = xt::fragment_count(len, t->X.max_payload);
  }
  if (!packed.empty()) HIP_TRY(hipMemcpy(t->d_store + t->store_used, packed.data(), packed.size(), hipMemcpyHostToDevice));
  t->store_used = at;
  if ((rc = put_words(t->X.file_off, t->h_off.data(), S)) != FSKHIP_OK || (rc = put_words(t->X.file_len, t->h_len.data(), S)) != FSKHIP_OK ||
      (rc = put_words(t->X.sequence, sequence.data(), S)) != FSKHIP_OK || (rc = put_words(t->X.index, index.data(), S)) != FSKHIP_OK ||
      (rc = put_words(t->X.n_fragments, n_fragments.data(), S)) != FSKHIP_OK || (rc = put_words(t->X.retries, retries.data(), S)) != FSKHIP_OK ||
      (rc = put_words(t->X.state, state.data(), S)) != FSKHIP_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_tx_reset(fskhip_xmodem_tx *t, int64_t stream) {
  if (!t) return fail(FSKHIP_E_INVALID, "null sender");
  if (stream >= (int64_t)t->p->S) return fail(FSKHIP_E_INVALID, "stream out of range");
  HIP_TRY(hipSetDevice(t->p->device));
  HIP_TRY(hipDeviceSynchronize());
  t->used = true;
  const size_t first = stream < 0 ? 0 : (size_t)stream, n = stream < 0 ? t->p->S : 1;
  uint32_t *zero[] = {t->X.state, t->X.index, t->X.n_fragments, t->X.retries, t->X.sent, t->X.retransmitted, t->X.file_off, t->X.file_len};
  for (uint32_t *z : zero)
    if (const int rc = fill_words(z + first, n, 0u)) return rc;
  if (const int rc = fill_words(t->X.sequence + first, n, 1u)) return rc;
  for (size_t s = first; s < first + n; s++) { t->h_off[s] = 0u; t->h_len[s] = 0u; t->h_has[s] = 0; }
  if (stream < 0) t->store_used = 0;   // (no file is left: the store starts over)
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_tx_state_get(fskhip_xmodem_tx *t, uint32_t *state, uint32_t *sequence, uint32_t *fragment_index, uint32_t *retries, uint32_t *packets_sent,
                               uint32_t *retransmitted) {
  if (!t) return fail(FSKHIP_E_INVALID, "null sender");
  HIP_TRY(hipSetDevice(t->p->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = sizeof(uint32_t) * t->p->S;
  const std::pair<uint32_t *, const uint32_t *> pairs[] = {{state, t->X.state}, {sequence, t->X.sequence}, {fragment_index, t->X.index}, {retries, t->X.retries},
                                                           {packets_sent, t->X.sent}, {retransmitted, t->X.retransmitted}};
  for (const auto &pr : pairs)
    if (pr.first && bytes) HIP_TRY(hipMemcpy(pr.first, pr.second, bytes, hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}

int fskhip_xmodem_tx_state_set(fskhip_xmodem_tx *t, const uint32_t *state, const uint32_t *sequence, const uint32_t *fragment_index, const uint32_t *retries,
                               const uint32_t *packets_sent, const uint32_t *retransmitted) {
  static const char fn[] = "fskhip_xmodem_tx_state_set";
  if (!t) return fail(FSKHIP_E_INVALID, "null sender");
  const size_t S = t->p->S;
  HIP_TRY(hipSetDevice(t->p->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> cur_state, cur_index;   // the values given take the place of the current ones
  int rc;
  if (!state && (rc = get_words(cur_state, t->X.state, S)) != FSKHIP_OK) return rc;
  if (!fragment_index && (rc = get_words(cur_index, t->X.index, S)) != FSKHIP_OK) return rc;
  for (size_t s = 0; s < S; s++) {
    const uint32_t st = state ? state[s] : cur_state[s], idx = fragment_index ? fragment_index[s] : cur_index[s];
    if (st > FSKHIP_XT_WAIT_FINAL_ACK) return fail(FSKHIP_E_INVALID, "%s: state[%zu] = %u is not a state (0-3)", fn, s, st);
    if (sequence && (sequence[s] < 1u || sequence[s] > 255u))
      return fail(FSKHIP_E_INVALID, "%s: sequence[%zu] = %u is not a sequence number (1-255)", fn, s, sequence[s]);
    const uint32_t n_frag = t->h_has[s] ? xt::fragment_count(t->h_len[s], t->X.max_payload) : 0u;
    if ((st == FSKHIP_XT_WAIT_NAK || st == FSKHIP_XT_WAIT_ACK) && idx >= n_frag)
      return fail(FSKHIP_E_INVALID, "%s: stream %zu waits to send fragment %u of %u", fn, s, idx, n_frag);
  }
  t->used = true;
  if ((rc = put_words(t->X.state, state, S)) != FSKHIP_OK || (rc = put_words(t->X.sequence, sequence, S)) != FSKHIP_OK ||
      (rc = put_words(t->X.index, fragment_index, S)) != FSKHIP_OK || (rc = put_words(t->X.retries, retries, S)) != FSKHIP_OK ||
      (rc = put_words(t->X.sent, packets_sent, S)) != FSKHIP_OK || (rc = put_words(t->X.retransmitted, retransmitted, S)) != FSKHIP_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_tx_poll_host(fskhip_xmodem_tx *t, const uint8_t *mask, const uint8_t *abort, uint32_t *streams, fskhip_xmodem_tx_event *events,
                               uint32_t cap_streams, uint32_t *n_events) {
  if (const int rc = poll_refusal("fskhip_xmodem_tx_poll_host", t, n_events, "n_events", streams, events, cap_streams)) return rc;
  fskhip_processor *p = t->p;
  p->used = true; t->used = true;
  *n_events = 0u;
  const size_t S = p->S;
  if (S == 0) return FSKHIP_OK;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  if (mask) HIP_TRY(hipMemcpy(t->d_mask, mask, S, hipMemcpyHostToDevice));
  if (abort) HIP_TRY(hipMemcpy(t->d_abort, abort, S, hipMemcpyHostToDevice));
  HIP_TRY(launch_xmodem_tx_step(p->T, p->S, mask ? t->d_mask : nullptr, abort ? t->d_abort : nullptr, t->X, t->W, cap_streams, t->d_totals, nullptr));
  uint32_t totals[3] = {0u, 0u, 0u};
  HIP_TRY(hipMemcpy(totals, t->d_totals, sizeof(totals), hipMemcpyDeviceToHost));
  *n_events = totals[0];
  if (totals[0] > cap_streams)
    return fail(FSKHIP_E_OVERFLOW, "%u streams have events, the lists hold %u streams (nothing was polled)", totals[0], cap_streams);
  int rc;   // staging for what is there; the commit also empties the rings of the streams whose reply held nothing for them
  if ((rc = ensure(t->d_streams, t->d_streams_cap, (size_t)totals[0] + 1)) != FSKHIP_OK) return rc;
  if ((rc = ensure(t->d_events, t->d_events_cap, (size_t)totals[0] + 1)) != FSKHIP_OK) return rc;
  HIP_TRY(launch_xmodem_tx_commit(p->T, p->S, t->X, t->W, t->d_totals, t->d_streams, t->d_events, nullptr));
  HIP_TRY(launch_processor_tx_start(p->e->M, p->T, t->W.slab, t->W.tx_lens, t->W.slab_pitch, t->W.tx_mask, nullptr));
  if (totals[0]) {
    HIP_TRY(hipMemcpy(streams, t->d_streams, sizeof(uint32_t) * totals[0], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(events, t->d_events, sizeof(fskhip_xmodem_tx_event) * totals[0], hipMemcpyDeviceToHost));
  } else {
    HIP_TRY(hipDeviceSynchronize());
  }
  return FSKHIP_OK;
}

int fskhip_xmodem_tx_poll_device(fskhip_xmodem_tx *t, const uint8_t *d_mask, const uint8_t *d_abort, uint32_t *d_streams, fskhip_xmodem_tx_event *d_events,
                                 uint32_t cap_streams, uint32_t *d_totals, void *hip_stream) {
  if (const int rc = poll_refusal("fskhip_xmodem_tx_poll_device", t, d_totals, "d_totals", d_streams, d_events, cap_streams)) return rc;
  fskhip_processor *p = t->p;
  p->used = true; t->used = true;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(launch_xmodem_tx_step(p->T, p->S, d_mask, d_abort, t->X, t->W, cap_streams, d_totals, st));
  HIP_TRY(launch_xmodem_tx_commit(p->T, p->S, t->X, t->W, d_totals, d_streams, d_events, st));
  if (p->S) HIP_TRY(launch_processor_tx_start(p->e->M, p->T, t->W.slab, t->W.tx_lens, t->W.slab_pitch, t->W.tx_mask, st));
  return FSKHIP_OK;
}

}  // extern "C"
