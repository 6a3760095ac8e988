// fsk_xmodem_recv_api.hip -- C ABI of the resident XModem file receiver (include/fskhip_next.h: fskhip_xmodem_recv_*): a handle
// over an FSKProcessor batch that keeps every stream's receive state, counters and assembled file on the device, polls the RX
// rings for the next step of receiveData() that owes a reply (fsk_xmodem_recv.hip) and starts the ACK / NAK on the processor.
// The timers and the decision to abort stay with the host, as masks.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "fsk_host.h"
#include "fsk_launch.h"
#include "fsk_proc.h"
#include "fsk_xmodem_handles.h"

using namespace fsk;

namespace {

const char *const kStateNames[] = {"IDLE", "RECEIVING_SEND_NAK", "RECEIVING_WAIT_BLOCK", "RECEIVING_SEND_ACK"};   // xmodem.ts:22-32
constexpr uint8_t kNAK = 0x15;

// what both forms of the poll refuse before they touch the device, in the header's order
int poll_refusal(const char *fn, const fskhip_xmodem_recv *r, const void *totals, const char *totals_name, const void *streams, const void *events,
                 uint32_t cap_streams) {
  if (!totals) return fail(FSKHIP_E_INVALID, "%s: null %s", fn, totals_name);
  if (cap_streams && (!streams || !events)) return fail(FSKHIP_E_INVALID, "%s: null streams or events with cap_streams %u", fn, cap_streams);
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  return FSKHIP_OK;
}

// sel and offsets of a files call on the device
int stage_lists(fskhip_xmodem_recv *r, const uint32_t *sel, const uint64_t *offsets, uint32_t n_sel) {
  int rc;
  if ((rc = ensure(r->d_sel, r->d_sel_cap, (size_t)n_sel)) != FSKHIP_OK) return rc;
  if ((rc = ensure(r->d_offsets, r->d_offsets_cap, (size_t)n_sel + 1)) != FSKHIP_OK) return rc;
  HIP_TRY(hipMemcpy(r->d_sel, sel, sizeof(uint32_t) * n_sel, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(r->d_offsets, offsets, sizeof(uint64_t) * ((size_t)n_sel + 1), hipMemcpyHostToDevice));
  return FSKHIP_OK;
}

}  // namespace

extern "C" {

int fskhip_xmodem_recv_destroy(fskhip_xmodem_recv *r) {
  if (!r) return FSKHIP_OK;
  xmodem_timers_orphan(r);
  (void)hipSetDevice(r->device);
  (void)hipDeviceSynchronize();
  void *bufs[] = {r->X.state, r->X.expected, r->X.retries, r->X.file_len, r->X.packets, r->X.dropped, r->X.sent, r->X.files,
                  r->W.ev, r->W.flags, r->W.removed, r->W.span, r->W.pairs, r->W.slab, r->W.tx_lens, r->W.tx_mask, r->d_totals,
                  r->d_mask, r->d_timeout, r->d_abort, r->d_streams, r->d_events, r->d_sel, r->d_offsets, r->d_packed};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  delete r;
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_create(fskhip_processor *p, uint32_t file_capacity, uint32_t max_retries, fskhip_xmodem_recv **out) {
  static const char fn[] = "fskhip_xmodem_recv_create";
  if (!p || !out) return fail(FSKHIP_E_INVALID, "%s: null argument", fn);
  if ((uint64_t)p->S * file_capacity > 0xFFFFFFFFull)
    return fail(FSKHIP_E_UNSUPPORTED, "%s: %u streams x file_capacity %u exceed the 32-bit offsets", fn, p->S, file_capacity);
  if ((uint64_t)p->S * p->T.rx_cap > 0xFFFFFFFFull)
    return fail(FSKHIP_E_UNSUPPORTED, "%s: %u streams x rx_capacity %u exceed the 32-bit offsets", fn, p->S, p->T.rx_cap);
  fskhip_xmodem_recv *r = new (std::nothrow) fskhip_xmodem_recv();
  if (!r) return fail(FSKHIP_E_NOMEM, "out of host memory");
  r->p = p;
  r->device = p->device;
  const size_t S = p->S;
  r->X.file_cap = file_capacity;
  r->X.max_retries = max_retries;
  r->W.slab_pitch = 16u;
  hipError_t herr = hipSetDevice(p->device);
  if (herr != hipSuccess) { delete r; return fail(FSKHIP_E_HIP, "hipSetDevice: %s", hipGetErrorString(herr)); }
  int rc = FSKHIP_OK;
#define XR_TRY(expr)                  \
  do {                                \
    if (rc == FSKHIP_OK) rc = (expr); \
  } while (0)
  uint32_t **words[] = {&r->X.state, &r->X.expected, &r->X.retries, &r->X.file_len, &r->X.packets, &r->X.dropped, &r->X.sent,
                        &r->W.flags, &r->W.removed, &r->W.span, &r->W.tx_lens};
  for (uint32_t **w : words) XR_TRY(dev_alloc(*w, S));
  XR_TRY(dev_alloc(r->X.files, S * (size_t)file_capacity));
  XR_TRY(dev_alloc(r->W.ev, S)); XR_TRY(dev_alloc(r->W.pairs, xmodem_recv_pair_words(p->S))); XR_TRY(dev_alloc(r->d_totals, 4));
  XR_TRY(dev_alloc(r->W.slab, S * r->W.slab_pitch)); XR_TRY(dev_alloc(r->W.tx_mask, S));
  XR_TRY(dev_alloc(r->d_mask, S)); XR_TRY(dev_alloc(r->d_timeout, S)); XR_TRY(dev_alloc(r->d_abort, S));
  XR_TRY(dev_alloc(r->d_streams, S)); XR_TRY(dev_alloc(r->d_events, S));
  if (rc == FSKHIP_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipDeviceSynchronize failed");
  for (uint32_t **w : words) XR_TRY(fill_words(*w, S, w == &r->X.expected ? 1u : 0u));
  if (rc == FSKHIP_OK && S && hipMemset(r->W.slab, 0, S * r->W.slab_pitch) != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipMemset failed");
  if (rc == FSKHIP_OK && S && file_capacity && hipMemset(r->X.files, 0, S * (size_t)file_capacity) != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipMemset failed");
  XR_TRY(processor_grow_payload(p, 1u));   // no poll ever needs to allocate
  if (rc == FSKHIP_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipDeviceSynchronize failed");
#undef XR_TRY
  if (rc != FSKHIP_OK) {
    const std::string keep = fskhip_last_error();
    fskhip_xmodem_recv_destroy(r);
    return fail(rc, "%s", keep.c_str());
  }
  *out = r;
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_start_host(fskhip_xmodem_recv *r, const uint8_t *mask) {
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  fskhip_processor *p = r->p;
  const size_t S = p->S;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> state, expected, retries, file_len, sent, pending;
  int rc;
  if ((rc = get_words(state, r->X.state, S)) != FSKHIP_OK || (rc = get_words(pending, p->T.tx_pending, S)) != FSKHIP_OK) return rc;
  for (size_t s = 0; s < S; s++)   // ensureIdle (xmodem.ts:571-575)
    if ((!mask || mask[s]) && state[s] != FSKHIP_XR_IDLE)
      return fail(FSKHIP_E_BUSY, "Transport busy: receiveData cannot start while in %s state (stream %zu)", kStateNames[state[s] & 3u], s);
  for (size_t s = 0; s < S; s++)
    if ((!mask || mask[s]) && pending[s]) return fail(FSKHIP_E_BUSY, "Modulation already in progress (stream %zu)", s);
  if (S == 0) return FSKHIP_OK;
  if ((rc = get_words(expected, r->X.expected, S)) != FSKHIP_OK || (rc = get_words(retries, r->X.retries, S)) != FSKHIP_OK ||
      (rc = get_words(file_len, r->X.file_len, S)) != FSKHIP_OK || (rc = get_words(sent, r->X.sent, S)) != FSKHIP_OK)
    return rc;
  p->used = true; r->used = true;
  std::vector<uint8_t> slab(S * r->W.slab_pitch, 0), tx_mask(S, 0);
  std::vector<uint32_t> lens(S, 0u);
  for (size_t s = 0; s < S; s++) {
    if (mask && !mask[s]) continue;
    state[s] = FSKHIP_XR_SEND_NAK; expected[s] = 1u; retries[s] = 0u; file_len[s] = 0u;   // initializeReceive (xmodem.ts:221-225)
    sent[s] += 1u;                                                                          // sendInitialNAK
    slab[s * r->W.slab_pitch] = kNAK; lens[s] = 1u; tx_mask[s] = 1;
  }
  if ((rc = put_words(r->X.state, state.data(), S)) != FSKHIP_OK || (rc = put_words(r->X.expected, expected.data(), S)) != FSKHIP_OK ||
      (rc = put_words(r->X.retries, retries.data(), S)) != FSKHIP_OK || (rc = put_words(r->X.file_len, file_len.data(), S)) != FSKHIP_OK ||
      (rc = put_words(r->X.sent, sent.data(), S)) != FSKHIP_OK || (rc = put_words(r->W.tx_lens, lens.data(), S)) != FSKHIP_OK)
    return rc;
  HIP_TRY(hipMemcpy(r->W.slab, slab.data(), slab.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(r->W.tx_mask, tx_mask.data(), S, hipMemcpyHostToDevice));
  HIP_TRY(launch_processor_tx_start(p->e->M, p->T, r->W.slab, r->W.tx_lens, r->W.slab_pitch, r->W.tx_mask, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_reset(fskhip_xmodem_recv *r, int64_t stream) {
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  if (stream >= (int64_t)r->p->S) return fail(FSKHIP_E_INVALID, "stream out of range");
  HIP_TRY(hipSetDevice(r->p->device));
  HIP_TRY(hipDeviceSynchronize());
  r->used = true;
  const size_t first = stream < 0 ? 0 : (size_t)stream, n = stream < 0 ? r->p->S : 1;
  uint32_t *zero[] = {r->X.state, r->X.retries, r->X.file_len, r->X.packets, r->X.dropped, r->X.sent};
  for (uint32_t *z : zero)
    if (const int rc = fill_words(z + first, n, 0u)) return rc;
  if (const int rc = fill_words(r->X.expected + first, n, 1u)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_state_get(fskhip_xmodem_recv *r, uint32_t *state, uint32_t *expected, uint32_t *retries, uint32_t *file_len, uint32_t *packets_received,
                                 uint32_t *dropped, uint32_t *packets_sent) {
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  HIP_TRY(hipSetDevice(r->p->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = sizeof(uint32_t) * r->p->S;
  const std::pair<uint32_t *, const uint32_t *> pairs[] = {{state, r->X.state}, {expected, r->X.expected}, {retries, r->X.retries}, {file_len, r->X.file_len},
                                                           {packets_received, r->X.packets}, {dropped, r->X.dropped}, {packets_sent, r->X.sent}};
  for (const auto &pr : pairs)
    if (pr.first && bytes) HIP_TRY(hipMemcpy(pr.first, pr.second, bytes, hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_state_set(fskhip_xmodem_recv *r, const uint32_t *state, const uint32_t *expected, const uint32_t *retries, const uint32_t *file_len,
                                 const uint32_t *packets_received, const uint32_t *dropped, const uint32_t *packets_sent) {
  static const char fn[] = "fskhip_xmodem_recv_state_set";
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  const size_t S = r->p->S;
  for (size_t s = 0; s < S; s++) {
    if (state && state[s] > FSKHIP_XR_SEND_ACK) return fail(FSKHIP_E_INVALID, "%s: state[%zu] = %u is not a state (0-3)", fn, s, state[s]);
    if (expected && (expected[s] < 1u || expected[s] > 255u))
      return fail(FSKHIP_E_INVALID, "%s: expected[%zu] = %u is not a sequence number (1-255)", fn, s, expected[s]);
    if (file_len && file_len[s] > r->X.file_cap)
      return fail(FSKHIP_E_INVALID, "%s: file_len[%zu] = %u exceeds file_capacity %u", fn, s, file_len[s], r->X.file_cap);
  }
  HIP_TRY(hipSetDevice(r->p->device));
  HIP_TRY(hipDeviceSynchronize());
  r->used = true;
  int rc;
  if ((rc = put_words(r->X.state, state, S)) != FSKHIP_OK || (rc = put_words(r->X.expected, expected, S)) != FSKHIP_OK ||
      (rc = put_words(r->X.retries, retries, S)) != FSKHIP_OK || (rc = put_words(r->X.file_len, file_len, S)) != FSKHIP_OK ||
      (rc = put_words(r->X.packets, packets_received, S)) != FSKHIP_OK || (rc = put_words(r->X.dropped, dropped, S)) != FSKHIP_OK ||
      (rc = put_words(r->X.sent, packets_sent, S)) != FSKHIP_OK)
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_files_host(fskhip_xmodem_recv *r, const uint32_t *sel, uint32_t n_sel, uint64_t *offsets, uint8_t *data, size_t cap_bytes,
                                  uint64_t *n_bytes) {
  static const char fn[] = "fskhip_xmodem_recv_files_host";
  if (!n_bytes) return fail(FSKHIP_E_INVALID, "%s: null n_bytes", fn);
  if (n_sel && (!sel || !offsets)) return fail(FSKHIP_E_INVALID, "%s: null sel or offsets with n_sel %u", fn, n_sel);
  if (cap_bytes && !data) return fail(FSKHIP_E_INVALID, "%s: null data with cap_bytes %zu", fn, cap_bytes);
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  const size_t S = r->p->S;
  for (uint32_t i = 0; i < n_sel; i++)
    if (sel[i] >= S) return fail(FSKHIP_E_INVALID, "%s: sel[%u] = %u is not a stream (%zu streams)", fn, i, sel[i], S);
  *n_bytes = 0u;
  if (offsets) offsets[0] = 0u;
  if (!n_sel) return FSKHIP_OK;
  HIP_TRY(hipSetDevice(r->p->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> file_len;
  int rc;
  if ((rc = get_words(file_len, r->X.file_len, S)) != FSKHIP_OK) return rc;
  for (uint32_t i = 0; i < n_sel; i++) offsets[i + 1] = offsets[i] + file_len[sel[i]];
  const uint64_t total = offsets[n_sel];
  *n_bytes = total;
  if (total > cap_bytes) return fail(FSKHIP_E_OVERFLOW, "the files hold %llu bytes, data holds %zu (nothing was copied)", (unsigned long long)total, cap_bytes);
  if (!total) return FSKHIP_OK;
  if ((rc = stage_lists(r, sel, offsets, n_sel)) != FSKHIP_OK) return rc;
  if ((rc = ensure(r->d_packed, r->d_packed_cap, (size_t)total)) != FSKHIP_OK) return rc;
  HIP_TRY(launch_xmodem_recv_files(true, r->X, r->d_sel, r->d_offsets, n_sel, r->d_packed, nullptr));
  HIP_TRY(hipMemcpy(data, r->d_packed, (size_t)total, hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_files_set_host(fskhip_xmodem_recv *r, const uint32_t *sel, uint32_t n_sel, const uint64_t *offsets, const uint8_t *data) {
  static const char fn[] = "fskhip_xmodem_recv_files_set_host";
  if (n_sel && (!sel || !offsets)) return fail(FSKHIP_E_INVALID, "%s: null sel or offsets with n_sel %u", fn, n_sel);
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  const size_t S = r->p->S;
  for (uint32_t i = 0; i < n_sel; i++) {
    if (sel[i] >= S) return fail(FSKHIP_E_INVALID, "%s: sel[%u] = %u is not a stream (%zu streams)", fn, i, sel[i], S);
    if (offsets[i] > offsets[i + 1]) return fail(FSKHIP_E_INVALID, "%s: offsets[%u] exceeds offsets[%u]", fn, i, i + 1);
    if (offsets[i + 1] - offsets[i] > r->X.file_cap)
      return fail(FSKHIP_E_INVALID, "%s: the file of stream %u has %llu bytes, file_capacity is %u", fn, sel[i],
                  (unsigned long long)(offsets[i + 1] - offsets[i]), r->X.file_cap);
    if (offsets[i + 1] > offsets[i] && !data) return fail(FSKHIP_E_INVALID, "%s: null data", fn);
  }
  r->used = true;
  if (!n_sel) return FSKHIP_OK;
  HIP_TRY(hipSetDevice(r->p->device));
  HIP_TRY(hipDeviceSynchronize());
  // the packed bytes as the kernel indexes them: from offsets[0] on
  const uint64_t first = offsets[0], total = offsets[n_sel] - first;
  std::vector<uint64_t> rel(offsets, offsets + n_sel + 1);
  for (uint64_t &o : rel) o -= first;
  int rc;
  if ((rc = stage_lists(r, sel, rel.data(), n_sel)) != FSKHIP_OK) return rc;
  if ((rc = ensure(r->d_packed, r->d_packed_cap, (size_t)total + 1)) != FSKHIP_OK) return rc;
  if (total) HIP_TRY(hipMemcpy(r->d_packed, data + first, (size_t)total, hipMemcpyHostToDevice));
  HIP_TRY(launch_xmodem_recv_files(false, r->X, r->d_sel, r->d_offsets, n_sel, r->d_packed, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_poll_host(fskhip_xmodem_recv *r, const uint8_t *mask, const uint8_t *timeout, const uint8_t *abort, uint32_t *streams,
                                 fskhip_xmodem_recv_event *events, uint32_t cap_streams, uint32_t *n_events) {
  if (const int rc = poll_refusal("fskhip_xmodem_recv_poll_host", r, n_events, "n_events", streams, events, cap_streams)) return rc;
  fskhip_processor *p = r->p;
  p->used = true; r->used = true;
  *n_events = 0u;
  const size_t S = p->S;
  if (S == 0) return FSKHIP_OK;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  if (mask) HIP_TRY(hipMemcpy(r->d_mask, mask, S, hipMemcpyHostToDevice));
  if (timeout) HIP_TRY(hipMemcpy(r->d_timeout, timeout, S, hipMemcpyHostToDevice));
  if (abort) HIP_TRY(hipMemcpy(r->d_abort, abort, S, hipMemcpyHostToDevice));
  HIP_TRY(launch_xmodem_recv_step(p->T, p->S, mask ? r->d_mask : nullptr, timeout ? r->d_timeout : nullptr, abort ? r->d_abort : nullptr, r->X, r->W,
                                  cap_streams, r->d_totals, nullptr));
  uint32_t totals[3] = {0u, 0u, 0u};
  HIP_TRY(hipMemcpy(totals, r->d_totals, sizeof(totals), hipMemcpyDeviceToHost));
  *n_events = totals[0];
  if (totals[0] > cap_streams)
    return fail(FSKHIP_E_OVERFLOW, "%u streams have events, the lists hold %u streams (nothing was polled)", totals[0], cap_streams);
  // (the commit also advances the rings of the streams that only swallowed noise)
  HIP_TRY(launch_xmodem_recv_commit(p->T, p->S, r->X, r->W, r->d_totals, r->d_streams, r->d_events, nullptr));
  HIP_TRY(launch_processor_tx_start(p->e->M, p->T, r->W.slab, r->W.tx_lens, r->W.slab_pitch, r->W.tx_mask, nullptr));
  if (totals[0]) {
    HIP_TRY(hipMemcpy(streams, r->d_streams, sizeof(uint32_t) * totals[0], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(events, r->d_events, sizeof(fskhip_xmodem_recv_event) * totals[0], hipMemcpyDeviceToHost));
  } else {
    HIP_TRY(hipDeviceSynchronize());
  }
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_poll_device(fskhip_xmodem_recv *r, const uint8_t *d_mask, const uint8_t *d_timeout, const uint8_t *d_abort, uint32_t *d_streams,
                                   fskhip_xmodem_recv_event *d_events, uint32_t cap_streams, uint32_t *d_totals, void *hip_stream) {
  if (const int rc = poll_refusal("fskhip_xmodem_recv_poll_device", r, d_totals, "d_totals", d_streams, d_events, cap_streams)) return rc;
  fskhip_processor *p = r->p;
  p->used = true; r->used = true;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(launch_xmodem_recv_step(p->T, p->S, d_mask, d_timeout, d_abort, r->X, r->W, cap_streams, d_totals, st));
  HIP_TRY(launch_xmodem_recv_commit(p->T, p->S, r->X, r->W, d_totals, d_streams, d_events, st));
  if (p->S) HIP_TRY(launch_processor_tx_start(p->e->M, p->T, r->W.slab, r->W.tx_lens, r->W.slab_pitch, r->W.tx_mask, st));
  return FSKHIP_OK;
}

}  // extern "C"
