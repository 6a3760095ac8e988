// fsk_xmodem_rx_api.hip -- C ABI of the resident XModem receiver (include/fskhip_next.h: fskhip_xmodem_rx_*): a handle over an
// FSKProcessor batch that keeps expectedSequence and the two running counters per stream on the device, and polls the RX rings
// in place (fsk_xmodem_rx.hip).  The control plane -- ACK / NAK, retries, timeouts -- stays with the host.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "fsk_host.h"
#include "fsk_launch.h"
#include "fsk_proc.h"
#include "fsk_xmodem_handles.h"

using namespace fsk;

namespace {

// what both forms of the poll refuse before they touch the device, in the header's order
int poll_refusal(const char *fn, const fskhip_xmodem_rx *r, const void *totals, const char *totals_name, const void *streams, const void *results,
                 const void *offsets, uint32_t cap_streams, const void *data, size_t cap_bytes) {
  if (!totals) return fail(FSKHIP_E_INVALID, "%s: null %s", fn, totals_name);
  if (cap_streams && (!streams || !results || !offsets))
    return fail(FSKHIP_E_INVALID, "%s: null streams, results or offsets with cap_streams %u", fn, cap_streams);
  if (cap_bytes && !data) return fail(FSKHIP_E_INVALID, "%s: null data with cap_bytes %zu", fn, cap_bytes);
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  if ((uint64_t)r->p->S * r->p->T.rx_cap > 0xFFFFFFFFull)
    return fail(FSKHIP_E_UNSUPPORTED, "%s: %u streams x rx_capacity %u exceed the 32-bit offsets", fn, r->p->S, r->p->T.rx_cap);
  return FSKHIP_OK;
}

}  // namespace

extern "C" {

int fskhip_xmodem_rx_destroy(fskhip_xmodem_rx *r) {
  if (!r) return FSKHIP_OK;
  (void)hipSetDevice(r->device);
  (void)hipDeviceSynchronize();
  void *bufs[] = {r->X.expected, r->X.packets, r->X.dropped, r->W.res, r->W.removed, r->W.flags, r->W.pairs, r->d_totals,
                  r->d_mask, r->d_lists, r->d_results, r->d_data};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  delete r;
  return FSKHIP_OK;
}

int fskhip_xmodem_rx_create(fskhip_processor *p, fskhip_xmodem_rx **out) {
  if (!p || !out) return fail(FSKHIP_E_INVALID, "fskhip_xmodem_rx_create: null argument");
  fskhip_xmodem_rx *r = new (std::nothrow) fskhip_xmodem_rx();
  if (!r) return fail(FSKHIP_E_NOMEM, "out of host memory");
  r->p = p;
  r->device = p->device;
  const size_t S = p->S;
  hipError_t herr = hipSetDevice(p->device);
  if (herr != hipSuccess) { delete r; return fail(FSKHIP_E_HIP, "hipSetDevice: %s", hipGetErrorString(herr)); }
  int rc = FSKHIP_OK;
#define RX_TRY(expr)                  \
  do {                                \
    if (rc == FSKHIP_OK) rc = (expr); \
  } while (0)
  RX_TRY(dev_alloc(r->X.expected, S)); RX_TRY(dev_alloc(r->X.packets, S)); RX_TRY(dev_alloc(r->X.dropped, S));
  RX_TRY(dev_alloc(r->W.res, S)); RX_TRY(dev_alloc(r->W.removed, S)); RX_TRY(dev_alloc(r->W.flags, S));
  RX_TRY(dev_alloc(r->W.pairs, xmodem_rx_pair_words(p->S))); RX_TRY(dev_alloc(r->d_totals, 4));
  RX_TRY(dev_alloc(r->d_mask, S));
  if (rc == FSKHIP_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipDeviceSynchronize failed");
  RX_TRY(fill_words(r->X.expected, S, 1u)); RX_TRY(fill_words(r->X.packets, S, 0u)); RX_TRY(fill_words(r->X.dropped, S, 0u));
  if (rc == FSKHIP_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipDeviceSynchronize failed");
#undef RX_TRY
  if (rc != FSKHIP_OK) {
    const std::string keep = fskhip_last_error();
    fskhip_xmodem_rx_destroy(r);
    return fail(rc, "%s", keep.c_str());
  }
  *out = r;
  return FSKHIP_OK;
}

int fskhip_xmodem_rx_reset(fskhip_xmodem_rx *r, int64_t stream) {
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  if (stream >= (int64_t)r->p->S) return fail(FSKHIP_E_INVALID, "stream out of range");
  HIP_TRY(hipSetDevice(r->p->device));
  HIP_TRY(hipDeviceSynchronize());
  r->used = true;
  const int rc = stream < 0 ? fill_words(r->X.expected, r->p->S, 1u) : fill_words(r->X.expected + stream, 1, 1u);
  if (rc != FSKHIP_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_rx_state_get(fskhip_xmodem_rx *r, uint32_t *expected, uint32_t *packets, uint32_t *dropped) {
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  HIP_TRY(hipSetDevice(r->p->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = sizeof(uint32_t) * r->p->S;
  if (expected && bytes) HIP_TRY(hipMemcpy(expected, r->X.expected, bytes, hipMemcpyDeviceToHost));
  if (packets && bytes) HIP_TRY(hipMemcpy(packets, r->X.packets, bytes, hipMemcpyDeviceToHost));
  if (dropped && bytes) HIP_TRY(hipMemcpy(dropped, r->X.dropped, bytes, hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}

int fskhip_xmodem_rx_state_set(fskhip_xmodem_rx *r, const uint32_t *expected, const uint32_t *packets, const uint32_t *dropped) {
  if (!r) return fail(FSKHIP_E_INVALID, "null receiver");
  if (expected)
    for (uint32_t s = 0; s < r->p->S; s++)
      if (expected[s] < 1u || expected[s] > 255u)
        return fail(FSKHIP_E_INVALID, "fskhip_xmodem_rx_state_set: expected[%u] = %u is not a sequence number (1-255)", s, expected[s]);
  HIP_TRY(hipSetDevice(r->p->device));
  HIP_TRY(hipDeviceSynchronize());
  r->used = true;
  const size_t bytes = sizeof(uint32_t) * r->p->S;
  if (expected && bytes) HIP_TRY(hipMemcpy(r->X.expected, expected, bytes, hipMemcpyHostToDevice));
  if (packets && bytes) HIP_TRY(hipMemcpy(r->X.packets, packets, bytes, hipMemcpyHostToDevice));
  if (dropped && bytes) HIP_TRY(hipMemcpy(r->X.dropped, dropped, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_rx_poll_host(fskhip_xmodem_rx *r, const uint8_t *mask, uint32_t *streams, fskhip_xmodem_result *results, uint32_t *offsets,
                               uint32_t cap_streams, uint8_t *data, size_t cap_bytes, uint32_t *n_events, uint32_t *n_bytes) {
  static const char fn[] = "fskhip_xmodem_rx_poll_host";
  if (const int rc = poll_refusal(fn, r, n_events && n_bytes ? (const void *)n_events : nullptr, "n_events or n_bytes", streams, results, offsets,
                                  cap_streams, data, cap_bytes))
    return rc;
  fskhip_processor *p = r->p;
  p->used = true; r->used = true;
  *n_events = 0u; *n_bytes = 0u;
  const size_t S = p->S;
  if (S == 0) {
    if (offsets) offsets[0] = 0u;
    return FSKHIP_OK;
  }
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  if (mask) HIP_TRY(hipMemcpy(r->d_mask, mask, S, hipMemcpyHostToDevice));
  const uint8_t *d_mask = mask ? r->d_mask : nullptr;
  HIP_TRY(launch_xmodem_rx_scan(p->T, p->S, d_mask, r->X, r->W, cap_streams, cap_bytes, r->d_totals, nullptr));
  uint32_t totals[2] = {0u, 0u};
  HIP_TRY(hipMemcpy(totals, r->d_totals, sizeof(totals), hipMemcpyDeviceToHost));
  *n_events = totals[0]; *n_bytes = totals[1];
  if (totals[0] > cap_streams || totals[1] > cap_bytes)
    return fail(FSKHIP_E_OVERFLOW, "%u streams have events with %u payload bytes, the lists hold %u streams and %zu bytes (nothing was polled)", totals[0],
                totals[1], cap_streams, cap_bytes);
  int rc;   // staging for what is there; the commit also advances the streams that only swallowed line noise
  if ((rc = ensure(r->d_data, r->d_data_cap, (size_t)totals[1] + 1)) != FSKHIP_OK) return rc;
  if ((rc = ensure(r->d_lists, r->d_lists_cap, 2 * (size_t)totals[0] + 1)) != FSKHIP_OK) return rc;
  if ((rc = ensure(r->d_results, r->d_results_cap, (size_t)totals[0] + 1)) != FSKHIP_OK) return rc;
  uint32_t *d_streams = r->d_lists, *d_offsets = r->d_lists + totals[0];
  HIP_TRY(launch_xmodem_rx_commit(p->T, p->S, r->X, r->W, r->d_totals, d_streams, r->d_results, d_offsets, r->d_data, nullptr));
  if (totals[0]) {
    HIP_TRY(hipMemcpy(streams, d_streams, sizeof(uint32_t) * totals[0], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(results, r->d_results, sizeof(fskhip_xmodem_result) * totals[0], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(offsets, d_offsets, sizeof(uint32_t) * ((size_t)totals[0] + 1), hipMemcpyDeviceToHost));
  } else {
    HIP_TRY(hipDeviceSynchronize());
    if (offsets) offsets[0] = 0u;
  }
  if (totals[1]) HIP_TRY(hipMemcpy(data, r->d_data, totals[1], hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}

int fskhip_xmodem_rx_poll_device(fskhip_xmodem_rx *r, const uint8_t *d_mask, uint32_t *d_streams, fskhip_xmodem_result *d_results, uint32_t *d_offsets,
                                 uint32_t cap_streams, uint8_t *d_data, size_t cap_bytes, uint32_t *d_totals, void *hip_stream) {
  if (const int rc = poll_refusal("fskhip_xmodem_rx_poll_device", r, d_totals, "d_totals", d_streams, d_results, d_offsets, cap_streams, d_data, cap_bytes))
    return rc;
  fskhip_processor *p = r->p;
  p->used = true; r->used = true;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(launch_xmodem_rx_scan(p->T, p->S, d_mask, r->X, r->W, cap_streams, cap_bytes, d_totals, st));
  HIP_TRY(launch_xmodem_rx_commit(p->T, p->S, r->X, r->W, d_totals, d_streams, d_results, d_offsets, d_data, st));
  return FSKHIP_OK;
}

}  // extern "C"
