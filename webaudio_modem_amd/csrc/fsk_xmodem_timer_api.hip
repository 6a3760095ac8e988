// fsk_xmodem_timer_api.hip -- C ABI of the resident XModem wait timers (include/fskhip_next.h: fskhip_xmodem_timer_*,
// fskhip_xmodem_recv_poll_timed_*, fskhip_xmodem_tx_poll_timed_*): a handle beside a file receiver or a sender that keeps every
// stream's wait timer on the device in the engine's sample clock and runs the handle's own poll between a fire and an arm pass
// (fsk_xmodem_timer.hip), so that the timeout and abort masks never exist on the host.  The external abort signal stays with the
// host, as the polls' abort mask.  The timers follow their streams through fskhip_xmodem_timer_remap, _snapshot
// and _restore: the two words move on the device (xm_timer_gather_kernel), an image ("FSKW") crosses PCIe once; its format and the
// one definition of a valid image are fsk_xmodem_timer_image.h's (host-only), and this file is the format's only writer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "fsk_engine.h"
#include "fsk_host.h"
#include "fsk_launch.h"
#include "fsk_proc.h"
#include "fsk_stage.h"
#include "fsk_xmodem_handles.h"
#include "fsk_xmodem_timer.h"
#include "fsk_xmodem_timer_image.h"

using namespace fsk;

struct fskhip_xmodem_timer {
  fskhip_xmodem_recv *r = nullptr;   // exactly one of the two
  fskhip_xmodem_tx *t = nullptr;
  bool orphan = false;               // the handle was destroyed first: every call but destroy is refused
  bool fresh = true;                 // no timed poll, reset or state_set call yet: what a remap or restore wants of its destination
  fskhip_processor *p = nullptr;
  int device = 0;
  uint32_t S = 0;
  XmTimerState W{};
  // staging for the _host forms, from create: no poll allocates
  uint8_t *d_mask = nullptr, *d_abort = nullptr;
  uint32_t *d_streams = nullptr, *d_totals = nullptr;
  void *d_events = nullptr;
};

namespace {

// the live timers, so that a handle's destroy can mark those over it
std::mutex g_lock;
std::vector<fskhip_xmodem_timer *> g_timers;

int usable(const char *fn, const fskhip_xmodem_timer *w) {
  if (!w) return fail(FSKHIP_E_INVALID, "%s: null timer", fn);
  std::lock_guard<std::mutex> hold(g_lock);
  if (w->orphan) return fail(FSKHIP_E_INVALID, "%s: the timer's %s has been destroyed", fn, w->r ? "receiver" : "sender");
  return FSKHIP_OK;
}

// what both forms of a timed poll refuse before they touch the device: the plain polls' refusals in their order, then the timer's
int poll_refusal(const char *fn, const fskhip_xmodem_timer *w, bool recv, const void *totals, const char *totals_name, const void *streams, const void *events,
                 uint32_t cap_streams) {
  if (!totals) return fail(FSKHIP_E_INVALID, "%s: null %s", fn, totals_name);
  if (cap_streams && (!streams || !events)) return fail(FSKHIP_E_INVALID, "%s: null streams or events with cap_streams %u", fn, cap_streams);
  if (const int rc = usable(fn, w)) return rc;
  if (recv != (w->r != nullptr)) return fail(FSKHIP_E_INVALID, "%s: the timer was created over a %s", fn, w->r ? "receiver" : "sender");
  return FSKHIP_OK;
}

int create(const char *fn, fskhip_xmodem_recv *r, fskhip_xmodem_tx *t, uint32_t timeout_samples, fskhip_xmodem_timer **out) {
  if ((!r && !t) || !out) return fail(FSKHIP_E_INVALID, "%s: null argument", fn);
  if (timeout_samples == 0u) return fail(FSKHIP_E_INVALID, "%s: timeout_samples is 0", fn);
  fskhip_xmodem_timer *w = new (std::nothrow) fskhip_xmodem_timer();
  if (!w) return fail(FSKHIP_E_NOMEM, "out of host memory");
  w->r = r; w->t = t;
  w->p = r ? r->p : t->p;
  w->device = w->p->device;
  w->S = w->p->S;
  w->W.timeout_samples = timeout_samples;
  const size_t S = w->S;
  hipError_t herr = hipSetDevice(w->device);
  if (herr != hipSuccess) { delete w; return fail(FSKHIP_E_HIP, "hipSetDevice: %s", hipGetErrorString(herr)); }
  int rc = FSKHIP_OK;
#define XW_TRY(expr)                  \
  do {                                \
    if (rc == FSKHIP_OK) rc = (expr); \
  } while (0)
  uint32_t **words[] = {&w->W.waited, &w->W.mark, &w->W.old_waited, &w->W.saved, &w->W.held, &w->d_streams};
  for (uint32_t **x : words) XW_TRY(dev_alloc(*x, S));
  XW_TRY(dev_alloc(w->W.flag, S)); XW_TRY(dev_alloc(w->d_mask, S)); XW_TRY(dev_alloc(w->d_abort, S)); XW_TRY(dev_alloc(w->d_totals, 4));
  uint8_t *events = nullptr;
  XW_TRY(dev_alloc(events, S * (r ? sizeof(fskhip_xmodem_recv_event) : sizeof(fskhip_xmodem_tx_event))));
  w->d_events = events;
  for (uint32_t **x : words) XW_TRY(fill_words(*x, S, 0u));
  if (rc == FSKHIP_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipDeviceSynchronize failed");
#undef XW_TRY
  if (rc != FSKHIP_OK) {
    const std::string keep = fskhip_last_error();
    fskhip_xmodem_timer_destroy(w);
    return fail(rc, "%s", keep.c_str());
  }
  {
    std::lock_guard<std::mutex> hold(g_lock);
    g_timers.push_back(w);
  }
  *out = w;
  return FSKHIP_OK;
}

// fire -> the handle's own poll -> arm, queued on `st`
int timed_recv(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *d_mask, const uint8_t *d_abort, uint32_t *d_streams, fskhip_xmodem_recv_event *d_events,
               uint32_t cap_streams, uint32_t *d_totals, hipStream_t st) {
  fskhip_xmodem_recv *r = w->r;
  w->fresh = false;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(launch_xmodem_timer_fire(w->W, true, r->X.state, w->p->T, w->S, d_mask, nullptr, elapsed, st));
  if (const int rc = fskhip_xmodem_recv_poll_device(r, d_mask, w->W.flag, d_abort, d_streams, d_events, cap_streams, d_totals, st)) return rc;
  HIP_TRY(launch_xmodem_timer_arm_recv(w->W, r->W.ev, w->p->T, w->S, d_totals, st));
  return FSKHIP_OK;
}

int timed_tx(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *d_mask, const uint8_t *d_abort, uint32_t *d_streams, fskhip_xmodem_tx_event *d_events,
             uint32_t cap_streams, uint32_t *d_totals, hipStream_t st) {
  fskhip_xmodem_tx *t = w->t;
  w->fresh = false;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(launch_xmodem_timer_fire(w->W, false, t->X.state, w->p->T, w->S, d_mask, d_abort, elapsed, st));
  if (const int rc = fskhip_xmodem_tx_poll_device(t, d_mask, w->W.flag, d_streams, d_events, cap_streams, d_totals, st)) return rc;
  HIP_TRY(launch_xmodem_timer_arm_tx(w->W, t->W.ev, w->p->T, w->S, d_totals, st));
  return FSKHIP_OK;
}

// the _host forms: masks up, the three passes on the null stream, then the totals and the lists down -- one synchronisation
template <class EV, class Run>
int timed_host(fskhip_xmodem_timer *w, const uint8_t *mask, const uint8_t *abort, uint32_t *streams, EV *events, uint32_t cap_streams, uint32_t *n_events, Run run) {
  *n_events = 0u;
  const size_t S = w->S;
  if (S == 0) return FSKHIP_OK;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipDeviceSynchronize());
  if (mask) HIP_TRY(hipMemcpy(w->d_mask, mask, S, hipMemcpyHostToDevice));
  if (abort) HIP_TRY(hipMemcpy(w->d_abort, abort, S, hipMemcpyHostToDevice));
  if (const int rc = run(mask ? w->d_mask : nullptr, abort ? w->d_abort : nullptr, w->d_streams, (EV *)w->d_events, w->d_totals)) return rc;
  uint32_t totals[3] = {0u, 0u, 0u};
  HIP_TRY(hipMemcpy(totals, w->d_totals, sizeof(totals), hipMemcpyDeviceToHost));
  *n_events = totals[0];
  if (totals[2] == 0u)
    return fail(FSKHIP_E_OVERFLOW, "%u streams have events, the lists hold %u streams (nothing was polled)", totals[0], cap_streams);
  if (totals[0]) {
    HIP_TRY(hipMemcpy(streams, w->d_streams, sizeof(uint32_t) * totals[0], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(events, w->d_events, sizeof(EV) * totals[0], hipMemcpyDeviceToHost));
  }
  return FSKHIP_OK;
}

uint32_t kind_of(const fskhip_xmodem_timer *w) { return w->r ? kXwKindRecv : kXwKindTx; }

// the last thing a remap or a restore asks of its destination.  (Neither call ends dst's freshness -- the header lists the calls
// that do --: they write every stream of dst, so a later one replaces the earlier one as a whole.)
int check_fresh(const char *who, const char *verb, const fskhip_xmodem_timer *dst) {
  if (!dst->fresh)
    return fail(FSKHIP_E_INVALID, "%s: the destination has been used already (timed poll, reset or state_set: %s into a freshly created timer)", who, verb);
  return FSKHIP_OK;
}

}  // namespace

namespace fsk {
void xmodem_timers_orphan(const void *handle) {
  std::lock_guard<std::mutex> hold(g_lock);
  for (fskhip_xmodem_timer *w : g_timers)
    if ((const void *)w->r == handle || (const void *)w->t == handle) w->orphan = true;
}
}  // namespace fsk

extern "C" {

int fskhip_xmodem_timer_create_recv(fskhip_xmodem_recv *r, uint32_t timeout_samples, fskhip_xmodem_timer **out) {
  return create("fskhip_xmodem_timer_create_recv", r, nullptr, timeout_samples, out);
}

int fskhip_xmodem_timer_create_tx(fskhip_xmodem_tx *t, uint32_t timeout_samples, fskhip_xmodem_timer **out) {
  return create("fskhip_xmodem_timer_create_tx", nullptr, t, timeout_samples, out);
}

int fskhip_xmodem_timer_destroy(fskhip_xmodem_timer *w) {
  if (!w) return FSKHIP_OK;
  {
    std::lock_guard<std::mutex> hold(g_lock);
    g_timers.erase(std::remove(g_timers.begin(), g_timers.end(), w), g_timers.end());
  }
  (void)hipSetDevice(w->device);
  (void)hipDeviceSynchronize();
  void *bufs[] = {w->W.waited, w->W.mark, w->W.old_waited, w->W.saved, w->W.held, w->W.flag, w->d_mask, w->d_abort, w->d_streams, w->d_totals, w->d_events};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  delete w;
  return FSKHIP_OK;
}

int fskhip_xmodem_timer_reset(fskhip_xmodem_timer *w, int64_t stream) {
  if (const int rc = usable("fskhip_xmodem_timer_reset", w)) return rc;
  if (stream >= (int64_t)w->S) return fail(FSKHIP_E_INVALID, "stream out of range");
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipDeviceSynchronize());
  w->fresh = false;
  const size_t first = stream < 0 ? 0 : (size_t)stream, n = stream < 0 ? w->S : 1;
  if (const int rc = fill_words(w->W.waited + first, n, 0u)) return rc;
  if (const int rc = fill_words(w->W.mark + first, n, 0u)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_timer_state_get(fskhip_xmodem_timer *w, uint32_t *waited, uint32_t *mark) {
  if (const int rc = usable("fskhip_xmodem_timer_state_get", w)) return rc;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = sizeof(uint32_t) * w->S;
  if (waited && bytes) HIP_TRY(hipMemcpy(waited, w->W.waited, bytes, hipMemcpyDeviceToHost));
  if (mark && bytes) HIP_TRY(hipMemcpy(mark, w->W.mark, bytes, hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}

int fskhip_xmodem_timer_state_set(fskhip_xmodem_timer *w, const uint32_t *waited, const uint32_t *mark) {
  static const char fn[] = "fskhip_xmodem_timer_state_set";
  if (const int rc = usable(fn, w)) return rc;
  for (size_t s = 0; mark && s < w->S; s++) {
    if (!xw::valid_mark(mark[s])) return fail(FSKHIP_E_INVALID, "%s: mark[%zu] = %u is not a mark (stage 0-2, plus 4 for was-pending)", fn, s, mark[s]);
    if (w->t && (mark[s] & xw::kStageMask)) return fail(FSKHIP_E_INVALID, "%s: mark[%zu] = %u has a stage, a sender's timer has none", fn, s, mark[s]);
  }
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipDeviceSynchronize());
  w->fresh = false;
  int rc;
  if ((rc = put_words(w->W.waited, waited, w->S)) != FSKHIP_OK || (rc = put_words(w->W.mark, mark, w->S)) != FSKHIP_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_xmodem_recv_poll_timed_device(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *d_mask, const uint8_t *d_abort, uint32_t *d_streams,
                                         fskhip_xmodem_recv_event *d_events, uint32_t cap_streams, uint32_t *d_totals, void *hip_stream) {
  if (const int rc = poll_refusal("fskhip_xmodem_recv_poll_timed_device", w, true, d_totals, "d_totals", d_streams, d_events, cap_streams)) return rc;
  return timed_recv(w, elapsed, d_mask, d_abort, d_streams, d_events, cap_streams, d_totals, (hipStream_t)hip_stream);
}

int fskhip_xmodem_recv_poll_timed_host(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *mask, const uint8_t *abort, uint32_t *streams,
                                       fskhip_xmodem_recv_event *events, uint32_t cap_streams, uint32_t *n_events) {
  if (const int rc = poll_refusal("fskhip_xmodem_recv_poll_timed_host", w, true, n_events, "n_events", streams, events, cap_streams)) return rc;
  return timed_host(w, mask, abort, streams, events, cap_streams, n_events,
                    [&](const uint8_t *m, const uint8_t *a, uint32_t *ds, fskhip_xmodem_recv_event *de, uint32_t *dt) {
                      return timed_recv(w, elapsed, m, a, ds, de, cap_streams, dt, nullptr);
                    });
}

int fskhip_xmodem_tx_poll_timed_device(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *d_mask, const uint8_t *d_abort, uint32_t *d_streams,
                                       fskhip_xmodem_tx_event *d_events, uint32_t cap_streams, uint32_t *d_totals, void *hip_stream) {
  if (const int rc = poll_refusal("fskhip_xmodem_tx_poll_timed_device", w, false, d_totals, "d_totals", d_streams, d_events, cap_streams)) return rc;
  return timed_tx(w, elapsed, d_mask, d_abort, d_streams, d_events, cap_streams, d_totals, (hipStream_t)hip_stream);
}

int fskhip_xmodem_tx_poll_timed_host(fskhip_xmodem_timer *w, uint32_t elapsed, const uint8_t *mask, const uint8_t *abort, uint32_t *streams,
                                     fskhip_xmodem_tx_event *events, uint32_t cap_streams, uint32_t *n_events) {
  if (const int rc = poll_refusal("fskhip_xmodem_tx_poll_timed_host", w, false, n_events, "n_events", streams, events, cap_streams)) return rc;
  return timed_host(w, mask, abort, streams, events, cap_streams, n_events,
                    [&](const uint8_t *m, const uint8_t *a, uint32_t *ds, fskhip_xmodem_tx_event *de, uint32_t *dt) {
                      return timed_tx(w, elapsed, m, a, ds, de, cap_streams, dt, nullptr);
                    });
}

// ---- remap, snapshot, restore ---------------------------------------------------------------------------------------------------
int fskhip_xmodem_timer_snapshot_info_get(const void *buf, size_t size, fskhip_xmodem_timer_snapshot_info *info) {
  static const char who[] = "fskhip_xmodem_timer_snapshot_info_get";
  XwImage im;
  if (const int rc = open_image(who, xw_image_open, buf, size, &im)) return rc;
  if (!info) return fail(FSKHIP_E_INVALID, "%s: null info", who);
  std::memset(info, 0, sizeof(*info));
  info->kind = im.h.kind; info->n_streams = im.h.n_records; info->timeout_samples = im.h.timeout_samples;
  return FSKHIP_OK;
}

int fskhip_xmodem_timer_remap(fskhip_xmodem_timer *dst, fskhip_xmodem_timer *src, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_xmodem_timer_remap";
  if (!dst || !src) return fail(FSKHIP_E_INVALID, "%s: null timer", who);
  if (dst == src) return fail(FSKHIP_E_INVALID, "%s: dst and src are the same timer", who);
  if (const int rc = usable(who, dst)) return rc;
  if (const int rc = usable(who, src)) return rc;
  if (const int rc = remap_check_map(who, "a source stream", map, n_map)) return rc;
  if (n_map != dst->S) return fail(FSKHIP_E_INVALID, "%s: n_map %u != the destination's %u streams", who, n_map, dst->S);
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] >= (int64_t)src->S) return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld, the source has %u streams", who, i, (long long)map[i], src->S);
  if (kind_of(dst) != kind_of(src))
    return fail(FSKHIP_E_INVALID, "%s: the timers are of different kinds (the destination's is over a %s, the source's over a %s)", who,
                dst->r ? "receiver" : "sender", src->r ? "receiver" : "sender");
  if (dst->device != src->device) return fail(FSKHIP_E_INVALID, "%s: the timers are on different devices (%d, %d): use a snapshot", who, dst->device, src->device);
  if (const int rc = check_fresh(who, "remap", dst)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  Scratch sc;
  int64_t *d_map = nullptr;
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  HIP_TRY(launch_xmodem_timer_gather(dst->W, src->W, d_map, n_map, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

size_t fskhip_xmodem_timer_snapshot_bytes(const fskhip_xmodem_timer *w, const int64_t *sel, uint32_t n_sel) {
  if (!w) return 0;
  return (size_t)xw_image_bytes(sel ? n_sel : w->S);
}

int fskhip_xmodem_timer_snapshot(fskhip_xmodem_timer *w, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written) {
  static const char who[] = "fskhip_xmodem_timer_snapshot";
  if (const int rc = usable(who, w)) return rc;
  if (!sel) n_sel = w->S;
  if (const int rc = check_sel(who, "timer", sel, n_sel, w->S)) return rc;
  const size_t need = (size_t)xw_image_bytes(n_sel);
  if (const int rc = check_room(who, n_sel, need, buf, cap, written)) return rc;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipDeviceSynchronize());
  XwImageHeader h = image_header<XwImageHeader>(kXwMagic, kXwFormat);
  h.kind = kind_of(w); h.n_records = n_sel; h.record_words = kXwRecordWords; h.timeout_samples = w->W.timeout_samples;
  const size_t body = need - sizeof(h), live = (size_t)xw_live_bytes(n_sel) - sizeof(h);
  Scratch sc;
  int64_t *d_sel = nullptr;
  uint8_t *d_body = nullptr;
  if (sel)
    if (const int rc = sc.upload(d_sel, sel, n_sel)) return rc;
  if (const int rc = sc.alloc(d_body, std::max<size_t>(body, 16))) return rc;
  if (body != live) HIP_TRY(hipMemset(d_body + live, 0, body - live));   // the padding behind an odd number of records
  HIP_TRY(launch_xmodem_timer_pack(w->W, d_sel, n_sel, (uint32_t *)d_body, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  unsigned char *out = (unsigned char *)buf;
  if (body) HIP_TRY(hipMemcpy(out + sizeof(h), d_body, body, hipMemcpyDeviceToHost));
  image_seal(h, out, need);
  return FSKHIP_OK;
}

int fskhip_xmodem_timer_restore(fskhip_xmodem_timer *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_xmodem_timer_restore";
  if (const int rc = usable(who, dst)) return rc;
  if (const int rc = remap_check_map(who, "a record of the snapshot", map, n_map)) return rc;
  XwImage im;
  if (const int rc = open_image(who, xw_image_open, buf, size, &im)) return rc;
  if (im.h.kind != kind_of(dst))
    return fail(FSKHIP_E_INVALID, "%s: the snapshot is of kind %u (%s), this timer's is %u (%s)", who, im.h.kind, xw_kind_name(im.h.kind), kind_of(dst),
                xw_kind_name(kind_of(dst)));
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] >= (int64_t)im.h.n_records)
      return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld, the snapshot has %u records", who, i, (long long)map[i], im.h.n_records);
  if (n_map != dst->S) return fail(FSKHIP_E_INVALID, "%s: n_map %u != the destination's %u streams", who, n_map, dst->S);
  if (const int rc = check_fresh(who, "restore", dst)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  Scratch sc;
  int64_t *d_map = nullptr;
  uint8_t *d_table = nullptr;
  const size_t table_bytes = (size_t)8u * im.h.n_records;
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  if (const int rc = sc.upload(d_table, (const uint8_t *)im.table, table_bytes)) return rc;
  HIP_TRY(launch_xmodem_timer_unpack(dst->W, (const uint32_t *)d_table, d_map, n_map, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

}  // extern "C"
