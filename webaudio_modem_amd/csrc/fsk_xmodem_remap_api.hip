// fsk_xmodem_remap_api.hip -- C ABI of libfskhip.so (include/fskhip_next.h): the three resident XModem handles carried through the
// lifecycle calls the engine and the processor row already have -- fskhip_xmodem_{rx,tx,recv}_remap, _snapshot_bytes, _snapshot,
// _restore, and fskhip_xmodem_snapshot_info_get for all three kinds of image.  A handle's per-stream words and its files (the
// sender's packed store, the file receiver's rows) move on the device (fsk_xmodem_remap.hip); an image crosses PCIe once.  The
// image's format and the one definition of a valid image are fsk_xmodem_image.h's (host-only, on fsk_image.h's frame); this file is
// the format's only writer.  The selection and room checks are fsk_stage.h's, the map's front check the engine remap's
// (remap_check_map), the per-call device scratch fsk_host.h's.
#include <algorithm>
#include <vector>

#include "fsk_engine.h"
#include "fsk_host.h"
#include "fsk_launch.h"
#include "fsk_proc.h"
#include "fsk_stage.h"
#include "fsk_xmodem_handles.h"
#include "fsk_xmodem_image.h"
#include "fsk_xmodem_tx_step.h"

using namespace fsk;

namespace {

// a handle's word arrays in the order of its image record, with what a new stream holds
XmWords words_of(const fskhip_xmodem_rx *r) {
  XmWords W{};
  W.a[0] = r->X.expected; W.a[1] = r->X.packets; W.a[2] = r->X.dropped;
  W.fresh[0] = 1u;
  W.n = 3u;
  return W;
}
// (the sender's file_len and has_file are the host's to set on a destination: `whole` adds them for a snapshot's pack)
XmWords words_of(const fskhip_xmodem_tx *t, bool whole) {
  XmWords W{};
  W.a[0] = t->X.state; W.a[1] = t->X.sequence; W.a[2] = t->X.index; W.a[3] = t->X.retries; W.a[4] = t->X.sent; W.a[5] = t->X.retransmitted;
  if (whole) { W.a[6] = t->X.file_len; W.a[7] = t->X.n_fragments; }
  W.fresh[1] = 1u;
  W.n = whole ? 8u : 6u;
  return W;
}
XmWords words_of(const fskhip_xmodem_recv *r) {
  XmWords W{};
  W.a[0] = r->X.state; W.a[1] = r->X.expected; W.a[2] = r->X.retries; W.a[3] = r->X.file_len; W.a[4] = r->X.packets; W.a[5] = r->X.dropped; W.a[6] = r->X.sent;
  W.fresh[1] = 1u;
  W.n = 7u;
  return W;
}

const char *fresh_text(uint32_t kind) {
  return kind == kXmKindRx ? "poll, reset or state_set" : kind == kXmKindTx ? "send, poll, reset or state_set" : "start, poll, reset, state_set or files_set";
}

// what a remap asks of its arguments before the kinds' own conditions.  (A remap or restore does not end dst's freshness -- the header
// lists the calls that do --: it writes every stream of dst, so a later one replaces the earlier one as a whole.)
template <class H>
int check_remap(const char *who, uint32_t kind, const H *dst, const H *src, const int64_t *map, uint32_t n_map) {
  if (!dst || !src) return fail(FSKHIP_E_INVALID, "%s: null handle", who);
  if (dst == src) return fail(FSKHIP_E_INVALID, "%s: dst and src are the same handle", who);
  if (const int rc = remap_check_map(who, "a source stream", map, n_map)) return rc;
  if (n_map != dst->p->S) return fail(FSKHIP_E_INVALID, "%s: n_map %u != the destination's %u streams", who, n_map, dst->p->S);
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] >= (int64_t)src->p->S) return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld, the source has %u streams", who, i, (long long)map[i], src->p->S);
  if (dst->device != src->device) return fail(FSKHIP_E_INVALID, "%s: the handles are on different devices (%d, %d): use a snapshot", who, dst->device, src->device);
  if (dst->used) return fail(FSKHIP_E_INVALID, "%s: the destination has been used already (%s: remap into a freshly created handle)", who, fresh_text(kind));
  return FSKHIP_OK;
}

// what a restore asks: the map's form, a valid image of the call's kind, entries that name records; then the destination
template <class H>
int check_restore(const char *who, uint32_t kind, const H *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map, XmImage *im) {
  if (const int rc = remap_check_map(who, "a record of the snapshot", map, n_map)) return rc;
  if (const int rc = open_image(who, xm_image_open, buf, size, im)) return rc;
  if (im->h.kind != kind)
    return fail(FSKHIP_E_INVALID, "%s: the snapshot is of kind %u (%s), this handle's is %u (%s)", who, im->h.kind, xm_kind_name(im->h.kind), kind, xm_kind_name(kind));
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] >= (int64_t)im->h.n_records)
      return fail(FSKHIP_E_INVALID, "%s: map[%u] = %lld, the snapshot has %u records", who, i, (long long)map[i], im->h.n_records);
  if (!dst) return fail(FSKHIP_E_INVALID, "%s: null handle", who);
  if (n_map != dst->p->S) return fail(FSKHIP_E_INVALID, "%s: n_map %u != the destination's %u streams", who, n_map, dst->p->S);
  if (dst->used) return fail(FSKHIP_E_INVALID, "%s: the destination has been used already (%s: restore into a freshly created handle)", who, fresh_text(kind));
  return FSKHIP_OK;
}

// the table and file area of a validated image on the device (both 16-byte aligned there)
int upload_image(Scratch &sc, const XmImage &im, size_t size, uint8_t *&d_img) {
  const size_t body = size - sizeof(XmImageHeader);
  if (const int rc = sc.alloc(d_img, std::max<size_t>(body, 16))) return rc;
  if (body) HIP_TRY(hipMemcpy(d_img, im.table, body, hipMemcpyHostToDevice));
  return FSKHIP_OK;
}
size_t table_bytes(const XmImageHeader &h) { return (size_t)4u * h.n_records * h.record_words; }

// the host's end of a snapshot: the body (table and file area, complete on the device) crosses in one copy, the header goes in front
int finish_snapshot(const char *who, XmImageHeader h, const uint8_t *d_body, void *buf, size_t need) {
  unsigned char *out = (unsigned char *)buf;
  const size_t body = need - sizeof(h);
  HIP_TRY(hipDeviceSynchronize());
  if (body) HIP_TRY_AS(hipMemcpy(out + sizeof(h), d_body, body, hipMemcpyDeviceToHost), who, false, (void)0);
  image_seal(h, out, need);
  return FSKHIP_OK;
}

XmImageHeader header_of(uint32_t kind, uint32_t n, uint32_t param0, uint32_t param1, uint64_t file_bytes) {
  XmImageHeader h = image_header<XmImageHeader>(kXmMagic, kXmFormat);
  h.kind = kind;
  h.n_records = n; h.record_words = xm_record_words(kind); h.param0 = param0; h.param1 = param1; h.file_bytes = file_bytes;
  return h;
}

// the body of an image on the device, its padding behind the files zeroed
int alloc_body(Scratch &sc, const XmImageHeader &h, uint8_t *&d_body) {
  const size_t tb = table_bytes(h), fb = (size_t)image_round16(h.file_bytes);
  if (const int rc = sc.alloc(d_body, std::max<size_t>(tb + fb, 16))) return rc;
  if (fb != h.file_bytes) HIP_TRY(hipMemset(d_body + tb + h.file_bytes, 0, fb - (size_t)h.file_bytes));
  return FSKHIP_OK;
}

// ---- the sender: its files' lengths and places are the host's -------------------------------------------------------------------
struct TxFile { uint8_t has; uint32_t len; uint64_t at; };   // a destination stream's file: held or not, its length, its place in the source's bytes

// dst takes the words through d_map (from src, or from record words on the device where src is null) and the files `f` out of
// d_src_bytes into a new, dense store.  Everything has been validated.  The files are copied into the new store first, and nothing of
// dst is written until that has succeeded: a failure up to there leaves dst as it was.  The words follow -- three host arrays and the
// gather, the gather last --; a HIP failure among those leaves dst's words partly written over its old store (the header says so:
// such a handle is to be destroyed).
int tx_carry(const char *who, fskhip_xmodem_tx *dst, Scratch &sc, const int64_t *d_map, const fskhip_xmodem_tx *src, const uint32_t *d_table,
             const std::vector<TxFile> &f, const uint8_t *d_src_bytes) {
  const uint32_t n = dst->p->S;
  uint64_t total = 0, longest = 0;
  for (const TxFile &x : f) { total += x.len; longest = std::max<uint64_t>(longest, x.len); }
  if (total > 0xFFFFFFFFull)
    return fail(FSKHIP_E_UNSUPPORTED, "%s: the carried files take %llu bytes, the store's offsets are 32-bit", who, (unsigned long long)total);
  std::vector<uint32_t> off(n, 0u), len(n, 0u), frag(n, 0u);
  std::vector<uint8_t> has(n, 0);
  std::vector<XmSpan> spans;
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!f[i].has) continue;
    has[i] = 1; off[i] = (uint32_t)at; len[i] = f[i].len; frag[i] = xt::fragment_count(f[i].len, dst->X.max_payload);
    if (f[i].len) spans.push_back(XmSpan{f[i].at, at, f[i].len});
    at += f[i].len;
  }
  const size_t cap = std::max<size_t>((size_t)image_round16(total), 4096);
  uint8_t *store = nullptr;
  if (const int rc = dev_alloc(store, cap)) return rc;
  XmSpan *d_spans = nullptr;
  int rc = sc.upload(d_spans, spans.data(), spans.size());
  const XmWords D = words_of(dst, false);
  XmWords S{};
  if (src) S = words_of(src, false);
  hipError_t err = hipSuccess;
  if (rc == FSKHIP_OK) err = launch_xmodem_span_copy(d_src_bytes, store, d_spans, (uint32_t)spans.size(), longest, nullptr);
  if (rc == FSKHIP_OK && err == hipSuccess) err = hipDeviceSynchronize();
  if (rc == FSKHIP_OK && err != hipSuccess) rc = fail(FSKHIP_E_HIP, "%s: %s", who, hipGetErrorString(err));
  // (from here on dst is written)
  if (rc == FSKHIP_OK) rc = put_words(dst->X.file_off, off.data(), n);
  if (rc == FSKHIP_OK) rc = put_words(dst->X.file_len, len.data(), n);
  if (rc == FSKHIP_OK) rc = put_words(dst->X.n_fragments, frag.data(), n);
  if (rc == FSKHIP_OK) {
    err = launch_xmodem_words_gather(D, n, d_map, src ? &S : nullptr, d_table, xm_record_words(kXmKindTx), nullptr);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) rc = fail(FSKHIP_E_HIP, "%s: %s", who, hipGetErrorString(err));
  }
  if (rc != FSKHIP_OK) { (void)hipDeviceSynchronize(); (void)hipFree(store); return rc; }
  if (dst->d_store) (void)hipFree(dst->d_store);
  dst->d_store = store; dst->store_cap = cap; dst->store_used = (size_t)total;
  dst->X.store = store;
  dst->h_off = off; dst->h_len = len; dst->h_has = has;
  return FSKHIP_OK;
}

// ---- the file receiver: file_len lives on the device ----------------------------------------------------------------------------
// d_offsets[0 .. n]: where each selected stream's file starts in a snapshot's file area; *total = all of them, *longest the longest
int recv_offsets(Scratch &sc, const fskhip_xmodem_recv *r, const int64_t *d_sel, uint32_t n, uint64_t *&d_offsets, uint64_t *total, uint64_t *longest) {
  uint64_t *d_sums = nullptr;
  if (const int rc = sc.alloc(d_offsets, (size_t)n + 1)) return rc;
  if (const int rc = sc.alloc(d_sums, xmodem_offsets_scratch_words(n))) return rc;
  HIP_TRY(launch_xmodem_file_offsets(r->X.file_len, d_sel, n, d_offsets, d_sums, nullptr));
  uint64_t ends[2] = {0u, 0u};   // (the scratch's last two words)
  HIP_TRY(hipMemcpy(ends, d_sums + xmodem_offsets_scratch_words(n) - 2, sizeof(ends), hipMemcpyDeviceToHost));
  *total = ends[0]; *longest = ends[1];
  return FSKHIP_OK;
}

template <class H>
int open_snapshot(const char *who, const H *h, const int64_t *&sel, uint32_t &n_sel) {
  if (!h) return fail(FSKHIP_E_INVALID, "%s: null handle", who);
  if (!sel) n_sel = h->p->S;
  if (const int rc = check_sel(who, "handle", sel, n_sel, h->p->S)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

uint64_t tx_file_bytes(const fskhip_xmodem_tx *t, const int64_t *sel, uint32_t n_sel) {
  uint64_t fb = 0;
  for (uint32_t r = 0; r < n_sel; r++) fb += t->h_len[sel ? (size_t)sel[r] : r];
  return fb;
}

}  // namespace

extern "C" {

int fskhip_xmodem_snapshot_info_get(const void *buf, size_t size, fskhip_xmodem_snapshot_info *info) {
  static const char who[] = "fskhip_xmodem_snapshot_info_get";
  XmImage im;
  if (const int rc = open_image(who, xm_image_open, buf, size, &im)) return rc;
  if (!info) return fail(FSKHIP_E_INVALID, "%s: null info", who);
  std::memset(info, 0, sizeof(*info));
  info->kind = im.h.kind; info->n_streams = im.h.n_records; info->param0 = im.h.param0; info->param1 = im.h.param1; info->file_bytes = im.h.file_bytes;
  return FSKHIP_OK;
}

// ---- rx -------------------------------------------------------------------------------------------------------------------------
int fskhip_xmodem_rx_remap(fskhip_xmodem_rx *dst, const fskhip_xmodem_rx *src, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_xmodem_rx_remap";
  if (const int rc = check_remap(who, kXmKindRx, dst, src, map, n_map)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  Scratch sc;
  int64_t *d_map = nullptr;
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  const XmWords S = words_of(src);
  HIP_TRY(launch_xmodem_words_gather(words_of(dst), n_map, d_map, &S, nullptr, 0u, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

size_t fskhip_xmodem_rx_snapshot_bytes(const fskhip_xmodem_rx *r, const int64_t *sel, uint32_t n_sel) {
  if (!r) return 0;
  if (!sel) n_sel = r->p->S;
  return xm_image_bytes(n_sel, xm_record_words(kXmKindRx), 0u);
}

int fskhip_xmodem_rx_snapshot(fskhip_xmodem_rx *r, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written) {
  static const char who[] = "fskhip_xmodem_rx_snapshot";
  if (const int rc = open_snapshot(who, r, sel, n_sel)) return rc;
  const XmImageHeader h = header_of(kXmKindRx, n_sel, 0u, 0u, 0u);
  const size_t need = xm_image_bytes(n_sel, h.record_words, 0u);
  if (const int rc = check_room(who, n_sel, need, buf, cap, written)) return rc;
  Scratch sc;
  int64_t *d_sel = nullptr;
  uint8_t *d_body = nullptr;
  if (sel)
    if (const int rc = sc.upload(d_sel, sel, n_sel)) return rc;
  if (const int rc = alloc_body(sc, h, d_body)) return rc;
  HIP_TRY(launch_xmodem_words_pack(words_of(r), d_sel, n_sel, h.record_words, false, (uint32_t *)d_body, nullptr));
  return finish_snapshot(who, h, d_body, buf, need);
}

int fskhip_xmodem_rx_restore(fskhip_xmodem_rx *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_xmodem_rx_restore";
  XmImage im;
  if (const int rc = check_restore(who, kXmKindRx, dst, buf, size, map, n_map, &im)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  Scratch sc;
  int64_t *d_map = nullptr;
  uint8_t *d_img = nullptr;
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  if (const int rc = upload_image(sc, im, size, d_img)) return rc;
  HIP_TRY(launch_xmodem_words_gather(words_of(dst), n_map, d_map, nullptr, (const uint32_t *)d_img, im.h.record_words, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

// ---- tx -------------------------------------------------------------------------------------------------------------------------
int fskhip_xmodem_tx_remap(fskhip_xmodem_tx *dst, const fskhip_xmodem_tx *src, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_xmodem_tx_remap";
  if (const int rc = check_remap(who, kXmKindTx, dst, src, map, n_map)) return rc;
  if (dst->X.max_payload != src->X.max_payload)
    return fail(FSKHIP_E_INVALID, "%s: max_payload_size differs (the destination's %u, the source's %u): a running transfer's fragments depend on it", who,
                dst->X.max_payload, src->X.max_payload);
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<TxFile> f(n_map, TxFile{0, 0u, 0u});
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] >= 0 && src->h_has[(size_t)map[i]]) f[i] = TxFile{1, src->h_len[(size_t)map[i]], src->h_off[(size_t)map[i]]};
  Scratch sc;
  int64_t *d_map = nullptr;
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  return tx_carry(who, dst, sc, d_map, src, nullptr, f, src->d_store);
}

size_t fskhip_xmodem_tx_snapshot_bytes(const fskhip_xmodem_tx *t, const int64_t *sel, uint32_t n_sel) {
  if (!t) return 0;
  if (!sel) n_sel = t->p->S;
  if (check_sel("fskhip_xmodem_tx_snapshot_bytes", "handle", sel, n_sel, t->p->S)) return 0;
  return xm_image_bytes(n_sel, xm_record_words(kXmKindTx), tx_file_bytes(t, sel, n_sel));
}

int fskhip_xmodem_tx_snapshot(fskhip_xmodem_tx *t, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written) {
  static const char who[] = "fskhip_xmodem_tx_snapshot";
  if (const int rc = open_snapshot(who, t, sel, n_sel)) return rc;
  const XmImageHeader h = header_of(kXmKindTx, n_sel, t->X.max_payload, t->X.max_retries, tx_file_bytes(t, sel, n_sel));
  const size_t need = xm_image_bytes(n_sel, h.record_words, h.file_bytes);
  if (const int rc = check_room(who, n_sel, need, buf, cap, written)) return rc;
  std::vector<XmSpan> spans;
  uint64_t at = 0, longest = 0;
  for (uint32_t r = 0; r < n_sel; r++) {
    const size_t s = sel ? (size_t)sel[r] : r;
    if (t->h_len[s]) spans.push_back(XmSpan{t->h_off[s], at, t->h_len[s]});
    at += t->h_len[s];
    longest = std::max<uint64_t>(longest, t->h_len[s]);
  }
  Scratch sc;
  int64_t *d_sel = nullptr;
  uint8_t *d_body = nullptr;
  XmSpan *d_spans = nullptr;
  if (sel)
    if (const int rc = sc.upload(d_sel, sel, n_sel)) return rc;
  if (const int rc = alloc_body(sc, h, d_body)) return rc;
  if (const int rc = sc.upload(d_spans, spans.data(), spans.size())) return rc;
  HIP_TRY(launch_xmodem_words_pack(words_of(t, true), d_sel, n_sel, h.record_words, true, (uint32_t *)d_body, nullptr));
  HIP_TRY(launch_xmodem_span_copy(t->d_store, d_body + table_bytes(h), d_spans, (uint32_t)spans.size(), longest, nullptr));
  return finish_snapshot(who, h, d_body, buf, need);
}

int fskhip_xmodem_tx_restore(fskhip_xmodem_tx *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_xmodem_tx_restore";
  XmImage im;
  if (const int rc = check_restore(who, kXmKindTx, dst, buf, size, map, n_map, &im)) return rc;
  if (dst->X.max_payload != im.h.param0)
    return fail(FSKHIP_E_INVALID, "%s: max_payload_size differs (the destination's %u, the snapshot's %u): a running transfer's fragments depend on it", who,
                dst->X.max_payload, im.h.param0);
  std::vector<uint64_t> rec_at((size_t)im.h.n_records + 1, 0u);
  for (uint32_t r = 0; r < im.h.n_records; r++) rec_at[r + 1] = rec_at[r] + im.file_len(r);
  std::vector<TxFile> f(n_map, TxFile{0, 0u, 0u});
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] >= 0 && im.word((uint32_t)map[i], 7u)) f[i] = TxFile{1, im.file_len((uint32_t)map[i]), rec_at[(size_t)map[i]]};
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  Scratch sc;
  int64_t *d_map = nullptr;
  uint8_t *d_img = nullptr;
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  if (const int rc = upload_image(sc, im, size, d_img)) return rc;
  return tx_carry(who, dst, sc, d_map, nullptr, (const uint32_t *)d_img, f, d_img + table_bytes(im.h));
}

// ---- recv -----------------------------------------------------------------------------------------------------------------------
int fskhip_xmodem_recv_remap(fskhip_xmodem_recv *dst, const fskhip_xmodem_recv *src, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_xmodem_recv_remap";
  if (const int rc = check_remap(who, kXmKindRecv, dst, src, map, n_map)) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  if (n_map == 0) return FSKHIP_OK;
  Scratch sc;
  int64_t *d_map = nullptr;
  XmSpan *d_spans = nullptr;
  uint32_t *d_bad = nullptr, plan[2] = {0u, 0u};   // the first stream whose file does not fit, the longest carried file
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  if (const int rc = sc.alloc(d_spans, n_map)) return rc;
  if (const int rc = sc.alloc(d_bad, 2)) return rc;
  // the spans go to scratch, so nothing of dst is written before every carried file is known to fit
  HIP_TRY(launch_xmodem_recv_plan(src->X.file_len, src->X.file_cap, dst->X.file_cap, d_map, n_map, d_spans, d_bad, nullptr));
  HIP_TRY(hipMemcpy(plan, d_bad, sizeof(plan), hipMemcpyDeviceToHost));
  if (const uint32_t bad = plan[0]; bad != 0xFFFFFFFFu) {
    uint32_t len = 0u;
    HIP_TRY(hipMemcpy(&len, src->X.file_len + map[bad], sizeof(len), hipMemcpyDeviceToHost));
    return fail(FSKHIP_E_INVALID, "%s: the file of stream %u (source stream %lld) has %u bytes, the destination's file_capacity is %u", who, bad,
                (long long)map[bad], len, dst->X.file_cap);
  }
  const XmWords S = words_of(src);
  HIP_TRY(launch_xmodem_words_gather(words_of(dst), n_map, d_map, &S, nullptr, 0u, nullptr));
  HIP_TRY(launch_xmodem_span_copy(src->X.files, dst->X.files, d_spans, n_map, plan[1], nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

size_t fskhip_xmodem_recv_snapshot_bytes(const fskhip_xmodem_recv *r, const int64_t *sel, uint32_t n_sel) {
  static const char who[] = "fskhip_xmodem_recv_snapshot_bytes";
  if (!r) return 0;
  if (open_snapshot(who, r, sel, n_sel)) return 0;
  Scratch sc;
  int64_t *d_sel = nullptr;
  uint64_t *d_offsets = nullptr, fb = 0, longest = 0;
  if (sel && sc.upload(d_sel, sel, n_sel)) return 0;
  if (recv_offsets(sc, r, d_sel, n_sel, d_offsets, &fb, &longest)) return 0;
  return xm_image_bytes(n_sel, xm_record_words(kXmKindRecv), fb);
}

int fskhip_xmodem_recv_snapshot(fskhip_xmodem_recv *r, const int64_t *sel, uint32_t n_sel, void *buf, size_t cap, size_t *written) {
  static const char who[] = "fskhip_xmodem_recv_snapshot";
  if (const int rc = open_snapshot(who, r, sel, n_sel)) return rc;
  Scratch sc;
  int64_t *d_sel = nullptr;
  uint64_t *d_offsets = nullptr, fb = 0, longest = 0;
  if (sel)
    if (const int rc = sc.upload(d_sel, sel, n_sel)) return rc;
  if (const int rc = recv_offsets(sc, r, d_sel, n_sel, d_offsets, &fb, &longest)) return rc;
  const XmImageHeader h = header_of(kXmKindRecv, n_sel, r->X.file_cap, r->X.max_retries, fb);
  const size_t need = xm_image_bytes(n_sel, h.record_words, fb);
  if (const int rc = check_room(who, n_sel, need, buf, cap, written)) return rc;
  uint8_t *d_body = nullptr;
  XmSpan *d_spans = nullptr;
  if (const int rc = alloc_body(sc, h, d_body)) return rc;
  if (const int rc = sc.alloc(d_spans, n_sel)) return rc;
  HIP_TRY(launch_xmodem_words_pack(words_of(r), d_sel, n_sel, h.record_words, false, (uint32_t *)d_body, nullptr));
  if (fb) {   // (a receiver whose files are all empty costs its word table)
    HIP_TRY(launch_xmodem_recv_spans(r->X.file_len, r->X.file_cap, d_sel, n_sel, d_offsets, d_spans, nullptr));
    HIP_TRY(launch_xmodem_span_copy(r->X.files, d_body + table_bytes(h), d_spans, n_sel, longest, nullptr));
  }
  return finish_snapshot(who, h, d_body, buf, need);
}

int fskhip_xmodem_recv_restore(fskhip_xmodem_recv *dst, const void *buf, size_t size, const int64_t *map, uint32_t n_map) {
  static const char who[] = "fskhip_xmodem_recv_restore";
  XmImage im;
  if (const int rc = check_restore(who, kXmKindRecv, dst, buf, size, map, n_map, &im)) return rc;
  std::vector<uint64_t> rec_at((size_t)im.h.n_records + 1, 0u);
  for (uint32_t r = 0; r < im.h.n_records; r++) rec_at[r + 1] = rec_at[r] + im.file_len(r);
  std::vector<XmSpan> spans;
  uint64_t longest = 0;
  for (uint32_t i = 0; i < n_map; i++) {
    if (map[i] < 0) continue;
    const uint32_t len = im.file_len((uint32_t)map[i]);
    if (len > dst->X.file_cap)
      return fail(FSKHIP_E_INVALID, "%s: the file of stream %u (record %lld) has %u bytes, the destination's file_capacity is %u", who, i, (long long)map[i], len,
                  dst->X.file_cap);
    if (len) spans.push_back(XmSpan{rec_at[(size_t)map[i]], (uint64_t)i * dst->X.file_cap, len});
    longest = std::max<uint64_t>(longest, len);
  }
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  if (n_map == 0) return FSKHIP_OK;
  Scratch sc;
  int64_t *d_map = nullptr;
  uint8_t *d_img = nullptr;
  XmSpan *d_spans = nullptr;
  if (const int rc = sc.upload(d_map, map, n_map)) return rc;
  if (const int rc = upload_image(sc, im, size, d_img)) return rc;
  if (const int rc = sc.upload(d_spans, spans.data(), spans.size())) return rc;
  HIP_TRY(launch_xmodem_words_gather(words_of(dst), n_map, d_map, nullptr, (const uint32_t *)d_img, im.h.record_words, nullptr));
  HIP_TRY(launch_xmodem_span_copy(d_img + table_bytes(im.h), dst->X.files, d_spans, (uint32_t)spans.size(), longest, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

}  // extern "C"
