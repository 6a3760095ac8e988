// fsk_addon_next.cc -- N-API binding of include/fskhip_next.h (CRC-16 / XModem packets, the FSKProcessor streaming
// contract, batched FIR), part of fsk_addon.node.  Same rules as fsk_addon.cc: typed arrays are borrowed for the
// call, results are fresh arrays, errors throw with the C library's message, nothing here computes.
// The helpers the entry points are spelled with (ARGS, typed, u32, index_array, ...) are addon_util.h's.
//
// JS surface added to the addon:
//   crc16(data: Uint8Array, pitch, lens: Uint32Array, device) -> Uint16Array
//   xmodemSerialize(payloads: Uint8Array, pitch, lens: Uint32Array, seqs: Uint32Array, device) -> {out, outPitch, lens}
//   xmodemScan(bytes: Uint8Array, pitch, counts: Uint32Array, expected: Uint32Array, device) -> {data, dataPitch, results: Int32Array[10*S]}
//   processorCreate(engine, rxCapacity) -> handle;  processorDestroy(handle)
//   processorProcess(handle, input: Float32Array|null, nIn, inPitch, nOut, flags) -> Float32Array|null
//   processorProcessSamples(handle, input: Float32Array|Int16Array|Uint8Array|null, inFormat, inLayout, nIn, inPitch, outFormat, outLayout,
//     nOut, outPitch, flags) -> the output format's typed array | null: the same with either side in a capture format and layout
//   processorModulate(handle, payloads: Uint8Array, lens: Uint32Array, pitch, mask: Uint8Array|null)
//   processorTxState(handle) -> {pos, total, pending, completed};  processorRxLength(handle) -> Uint32Array
//   processorLastTxKernel(handle) -> string
//   processorDrain(handle, capacity) -> {out, outPitch, counts};  processorReset(handle, stream)
//   processorDrainSparse(handle, mask: Uint8Array|null, minLen) -> {streams: Uint32Array, offsets: Uint32Array, data: Uint8Array}
//   xmodemRxCreate(processor) -> handle;  xmodemRxDestroy(handle);  xmodemRxReset(handle, stream)
//   xmodemRxPoll(handle, mask: Uint8Array|null) -> {streams: Uint32Array, results: Int32Array[10*n], offsets: Uint32Array, data: Uint8Array}
//   xmodemRxState(handle) -> {expected, packets, dropped: Uint32Array};  xmodemRxSetState(handle, expected|null, packets|null, dropped|null)
//   xmodemTxCreate(processor, maxPayloadSize, maxRetries) -> handle;  xmodemTxDestroy(handle);  xmodemTxReset(handle, stream)
//   xmodemTxSend(handle, mask: Uint8Array|null, offsets: Uint32Array[nStreams + 1], data: Uint8Array)
//   xmodemTxPoll(handle, mask: Uint8Array|null, abort: Uint8Array|null) -> {streams: Uint32Array, events: Int32Array[8*n]}
//   xmodemTxState(handle) -> {state, sequence, fragmentIndex, retries, packetsSent, retransmitted: Uint32Array};  xmodemTxSetState(handle, the six|null)
//   xmodemRecvCreate(processor, fileCapacity, maxRetries) -> handle;  xmodemRecvDestroy(handle);  xmodemRecvReset(handle, stream)
//   xmodemRecvStart(handle, mask: Uint8Array|null)
//   xmodemRecvPoll(handle, mask, timeout, abort: Uint8Array|null) -> {streams: Uint32Array, events: Int32Array[12*n]}
//   xmodemRecvFiles(handle, sel: Uint32Array) -> {offsets: Float64Array[n + 1], data: Uint8Array}
//   xmodemRecvSetFiles(handle, sel: Uint32Array, offsets: Uint32Array[n + 1], data: Uint8Array)
//   xmodemRecvState(handle) -> {state, expected, retries, fileLen, packetsReceived, dropped, packetsSent: Uint32Array};  xmodemRecvSetState(handle, the seven|null)
//   xmodemTimerCreate(overReceiver: boolean, recv or tx handle, timeoutSamples) -> handle;  xmodemTimerDestroy(handle);  xmodemTimerReset(handle, stream)
//   xmodemTimerPoll(handle, elapsed, mask, abort: Uint8Array|null) -> what xmodemRecvPoll / xmodemTxPoll return
//   xmodemTimerState(handle) -> {waited, mark: Uint32Array};  xmodemTimerSetState(handle, waited|null, mark|null)
//   xmodem{Rx,Tx,Recv}Remap(dst, src, map: number[]);  xmodem{Rx,Tx,Recv}Snapshot(handle, sel: number[]|null) -> Buffer
//   xmodem{Rx,Tx,Recv}Restore(dst, snapshot: Uint8Array, map: number[]);  xmodemSnapshotInfo(snapshot) -> {kind, nStreams, param0, param1, fileBytes}
//   processorRemap(dst, src, map: number[]);  processorSnapshot(handle, sel: number[]|null) -> Buffer
//   processorRestore(dst, snapshot: Uint8Array, map: number[]);  processorSnapshotInfo(snapshot) -> {nStreams, rxCapacity, payloadCapacity, recordBytes}
//   sincLowpass/sincHighpass(cutoff, sampleRate, numTaps), sincBandpass(center, bandwidth, sampleRate, numTaps) -> Float64Array
//   firCreate(taps: Float64Array, nStreams, device, precision) -> handle;  firDestroy(handle)
//   firProcess(handle, input: Float32Array, n, pitch, nStreams) -> Float32Array;  firReset(handle, stream)
//   resamplerCreate(direction, factor, taps: Float64Array, nStreams, device, precision) -> handle;  resamplerDestroy(handle);  resamplerHistory(handle);  resamplerStreams(handle)
//   resamplerUp(handle, samples, format, layout, nIn, pitch, factor) -> Float32Array [S][nIn * factor]
//   resamplerDown(handle, input: Float32Array [S][nIn], nIn, lens: Uint32Array|null, format, layout, factor) -> the format's typed array
//   processorProcessSamplesAt(handle, up: resampler handle|null, down: resampler handle|null, input, inFormat, inLayout, nIn, inPitch, outFormat,
//     outLayout, nOut, outPitch, flags) -> as processorProcessSamples, both sides at the handles' low rate (a side without samples needs none)
//   resamplerReset(handle, stream);  resamplerState(handle) -> Float32Array [S][history];  resamplerSetState(handle, Float32Array)
//   resamplerRemap(handle, map: number[]) -> handle;  resamplerSnapshot(handle, streams: number[]|null) -> Buffer
//   resamplerRestore(snapshot: Uint8Array, map: number[]|null, device) -> handle
//   resamplerSnapshotInfo(snapshot) -> {nStreams, direction, factor, nTaps, precision, history, taps: Float64Array}
//   ratecvtCreate(direction, up, down, taps: Float64Array, nStreams, device, precision) -> handle;  ratecvtDestroy(handle);  ratecvtHistory(handle);  ratecvtStreams(handle)
//   ratecvtCapture(handle, samples, format, layout, nIn, pitch, nOut) -> Float32Array [S][nOut]
//   ratecvtPlayback(handle, input: Float32Array [S][nIn], nIn, lens: Uint32Array|null, format, layout, nOut) -> the format's typed array
//   ratecvtReset(handle, stream);  ratecvtState(handle) -> Float32Array [S][history];  ratecvtSetState(handle, Float32Array)
//   ratecvtCaptureAny / ratecvtPlaybackAny: the two process calls for any nIn, from the handle's position (nOut: ratecvtOutCountAny's)
//   ratecvtPosition(handle) -> number;  ratecvtSetPosition(handle, pos);  ratecvtOutCountAny(handle, nIn);  ratecvtInCountAny(handle, nOut)
//   ratecvtRemap(handle, map: number[]) -> handle;  ratecvtSnapshot(handle, streams: number[]|null) -> Buffer
//   ratecvtRestore(snapshot: Uint8Array, map: number[]|null, device) -> handle
//   ratecvtSnapshotInfo(snapshot) -> {nStreams, direction, up, down, nTaps, precision, history, position, taps: Float64Array}
//   processorProcessSamplesAtAny: processorProcessSamplesAt for rate converters and counts of any length
//   iirCreate(b, a: Float64Array, nStreams, device, precision) -> handle; iirProcess(handle, Float32Array | Float64Array, n, pitch, nStreams);
//   iirCoefficients(handle), iirReset(handle, stream), iirDestroy(handle); butterworth(kind, f, bandwidth, sampleRate) -> [b0 b1 b2 a0 a1 a2]
#include <cstring>
#include <vector>

#include "../include/fskhip_next.h"
#include "addon_util.h"

namespace {

// FIR / IIR filter and resampler handles: the external owns a box, so that close() can empty it (a later call throws instead of
// touching freed memory) and a filter that is never close()d is destroyed when the garbage collector drops the handle
enum { BOX_FIR = 0, BOX_IIR = 1, BOX_RESAMPLER = 2, BOX_RATECVT = 3 };
struct FilterBox { void *p; int kind; };
void filter_box_destroy(FilterBox *b) {
  if (!b->p) return;
  if (b->kind == BOX_IIR) fskhip_iir_destroy((fskhip_iir *)b->p);
  else if (b->kind == BOX_RESAMPLER) fskhip_resampler_destroy((fskhip_resampler *)b->p);
  else if (b->kind == BOX_RATECVT) fskhip_ratecvt_destroy((fskhip_ratecvt *)b->p);
  else fskhip_fir_destroy((fskhip_fir *)b->p);
  b->p = nullptr;
}
void filter_box_finalize(napi_env, void *data, void *) {
  FilterBox *b = (FilterBox *)data;
  filter_box_destroy(b);
  delete b;
}
napi_value filter_box_new(napi_env env, void *p, int kind) {
  FilterBox *b = new FilterBox{p, kind};
  napi_value ext;
  if (napi_create_external(env, b, filter_box_finalize, nullptr, &ext) != napi_ok) { filter_box_finalize(env, b, nullptr); return nullptr; }
  return ext;
}
void *filter_of(napi_env env, napi_value v) {
  FilterBox *b = (FilterBox *)external(env, v, "filter destroyed");
  if (!b) return nullptr;
  if (!b->p) { napi_throw_error(env, nullptr, "filter destroyed"); return nullptr; }
  return b->p;
}
void filter_box_close(napi_env env, napi_value v) {
  void *q = nullptr;
  if (napi_get_value_external(env, v, &q) != napi_ok || !q) return;
  filter_box_destroy((FilterBox *)q);
}
napi_value Crc16(napi_env env, napi_callback_info info) {
  ARGS(4);
  void *data, *lens; size_t dlen, llen;
  if (!typed(env, argv[0], napi_uint8_array, &data, &dlen) || !typed(env, argv[2], napi_uint32_array, &lens, &llen)) return nullptr;
  const uint32_t pitch = u32(env, argv[1]);
  if ((size_t)pitch * llen > dlen) { napi_throw_range_error(env, nullptr, "data too short"); return nullptr; }
  void *out;
  napi_value out_v = make_typed(env, napi_uint16_array, llen, 2, &out);
  int rc = fskhip_crc16_host(i32(env, argv[3]), (const uint8_t *)data, pitch, (const uint32_t *)lens, (uint32_t)llen, (uint16_t *)out);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return out_v;
}

napi_value XmodemSerialize(napi_env env, napi_callback_info info) {
  ARGS(5);
  void *pl, *lens, *seqs; size_t plen, llen, slen;
  if (!typed(env, argv[0], napi_uint8_array, &pl, &plen) || !typed(env, argv[2], napi_uint32_array, &lens, &llen) ||
      !typed(env, argv[3], napi_uint32_array, &seqs, &slen)) return nullptr;
  const uint32_t pitch = u32(env, argv[1]);
  if (slen < llen || (size_t)pitch * llen > plen) { napi_throw_range_error(env, nullptr, "arguments too short"); return nullptr; }
  uint32_t mx = 0;
  for (size_t i = 0; i < llen; i++) mx = ((uint32_t *)lens)[i] > mx ? ((uint32_t *)lens)[i] : mx;
  const size_t out_pitch = (size_t)mx + 6;
  void *out, *olens;
  napi_value out_v = make_typed(env, napi_uint8_array, out_pitch * llen, 1, &out);
  napi_value len_v = make_typed(env, napi_uint32_array, llen, 4, &olens);
  int rc = fskhip_xmodem_serialize_host(i32(env, argv[4]), (const uint8_t *)pl, pitch, (const uint32_t *)lens, (const uint32_t *)seqs,
                                        (uint32_t)llen, (uint8_t *)out, out_pitch, (uint32_t *)olens);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value res;
  NAPI_OK(napi_create_object(env, &res));
  napi_set_named_property(env, res, "out", out_v);
  napi_set_named_property(env, res, "lens", len_v);
  set_u32(env, res, "outPitch", (uint32_t)out_pitch);
  return res;
}

napi_value XmodemScan(napi_env env, napi_callback_info info) {
  ARGS(5);
  void *bytes, *counts, *expected; size_t blen, clen, elen;
  if (!typed(env, argv[0], napi_uint8_array, &bytes, &blen) || !typed(env, argv[2], napi_uint32_array, &counts, &clen) ||
      !typed(env, argv[3], napi_uint32_array, &expected, &elen)) return nullptr;
  const uint32_t pitch = u32(env, argv[1]);
  if (elen < clen || (size_t)pitch * clen > blen) { napi_throw_range_error(env, nullptr, "arguments too short"); return nullptr; }
  const size_t data_pitch = pitch ? pitch : 4;
  static_assert(sizeof(fskhip_xmodem_result) == 40, "result layout");
  void *data, *res;
  napi_value data_v = make_typed(env, napi_uint8_array, data_pitch * clen, 1, &data);
  napi_value res_v = make_typed(env, napi_int32_array, 10 * clen, 4, &res);
  int rc = fskhip_xmodem_scan_host(i32(env, argv[4]), (const uint8_t *)bytes, pitch, (const uint32_t *)counts, (const uint32_t *)expected,
                                   (uint32_t)clen, (uint8_t *)data, data_pitch, (fskhip_xmodem_result *)res);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "data", data_v);
  napi_set_named_property(env, o, "results", res_v);
  set_u32(env, o, "dataPitch", (uint32_t)data_pitch);
  return o;
}

// ---- FSKProcessor -----------------------------------------------------------------------------------
struct Proc { fskhip_processor *p; uint32_t S; };

napi_value ProcessorCreate(napi_env env, napi_callback_info info) {
  ARGS(2);
  fskhip_engine *e = (fskhip_engine *)external(env, argv[0], "FSK modulator not configured");
  if (!e) return nullptr;
  fskhip_processor *p = nullptr;
  int rc = fskhip_processor_create(e, u32(env, argv[1]), &p);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  Proc *h = new Proc{p, fskhip_n_streams(e)};
  napi_value ext;
  NAPI_OK(napi_create_external(env, h, nullptr, nullptr, &ext));
  return ext;
}
napi_value ProcessorDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  void *p = nullptr;
  if (napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
    Proc *h = (Proc *)p;
    if (h->p) fskhip_processor_destroy(h->p);
    h->p = nullptr;
  }
  return nullptr;
}
Proc *get_proc(napi_env env, napi_value v) {
  Proc *h = (Proc *)external(env, v, "processor destroyed");
  if (h && !h->p) { napi_throw_error(env, nullptr, "processor destroyed"); return nullptr; }
  return h;
}

// the array a process call writes: the caller's `v` -- an optional last argument, which a sharded batch uses to let every shard
// write its block of ONE array: of the output's type and at least `need` elements, returned as it is -- or, where v is absent or
// null, a new one of `need` elements.  nullptr: thrown.
static napi_value output_array(napi_env env, bool given, napi_value v, napi_typedarray_type type, size_t need, size_t elem, void **out, bool *fresh) {
  *fresh = !given || nullish(env, v);
  if (*fresh) {
    napi_value o = make_typed(env, type, need, elem, out);
    if (!o) napi_throw_error(env, nullptr, "allocation failed");
    return o;
  }
  size_t len = 0;
  if (!typed(env, v, type, out, &len)) return nullptr;
  if (len < need) { napi_throw_range_error(env, nullptr, "out too short"); return nullptr; }
  return v;
}

napi_value ProcessorProcess(napi_env env, napi_callback_info info) {
  ARGS_UPTO(7);
  if (argc < 6) { napi_throw_type_error(env, nullptr, "too few arguments"); return nullptr; }
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  void *in; size_t ilen;
  if (!typed(env, argv[1], napi_float32_array, &in, &ilen, true)) return nullptr;
  const uint32_t n_in = u32(env, argv[2]), in_pitch = u32(env, argv[3]), n_out = u32(env, argv[4]), flags = u32(env, argv[5]);
  if (in && (in_pitch < n_in || (size_t)in_pitch * (h->S - 1) + n_in > ilen)) { napi_throw_range_error(env, nullptr, "input too short"); return nullptr; }
  void *out = nullptr;
  napi_value out_v = nullptr;
  bool fresh = true;
  if (n_out && !(out_v = output_array(env, argc > 6, argv[6], napi_float32_array, (size_t)n_out * h->S, 4, &out, &fresh))) return nullptr;
  int rc = fskhip_processor_process_host(h->p, (float *)in, n_in, in_pitch, (float *)out, n_out, n_out, flags);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  if (!out_v) napi_get_null(env, &out_v);
  return out_v;
}

// elements a [rows][pitch] array of rows x cols samples needs (the last row may end with its own samples); -1: pitch < cols
static inline int64_t samples_needed(int32_t layout, uint32_t S, uint32_t n, uint32_t pitch) {
  const size_t rows = layout == FSKHIP_LAYOUT_SAMPLE_MAJOR ? n : S, cols = layout == FSKHIP_LAYOUT_SAMPLE_MAJOR ? S : n;
  if (pitch < cols) return -1;
  return rows ? (int64_t)pitch * (int64_t)(rows - 1) + (int64_t)cols : 0;
}

// process() with either side in a capture format and layout (fskhip_processor_process_fmt_host): the input is the input format's
// typed array or null, the result a new array of the output format's type, [S][outPitch] or [nOut][outPitch >= S] (its padding the
// format's silence), or null when nOut is 0
napi_value ProcessorProcessSamples(napi_env env, napi_callback_info info) {
  ARGS_UPTO(12);
  if (argc < 11) { napi_throw_type_error(env, nullptr, "too few arguments"); return nullptr; }
  const int32_t in_format = i32(env, argv[2]), in_layout = i32(env, argv[3]), out_format = i32(env, argv[6]), out_layout = i32(env, argv[7]);
  if (!sample_format_ok(env, in_format, in_layout) || !sample_format_ok(env, out_format, out_layout)) return nullptr;
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  void *in; size_t ilen;
  if (!typed(env, argv[1], sample_array_type(in_format), &in, &ilen, true)) return nullptr;
  const uint32_t n_in = u32(env, argv[4]), in_pitch = u32(env, argv[5]), n_out = u32(env, argv[8]), out_pitch = u32(env, argv[9]), flags = u32(env, argv[10]);
  if (in) {
    const int64_t need = samples_needed(in_layout, h->S, n_in, in_pitch);
    if (need < 0 || (size_t)need > ilen) { napi_throw_range_error(env, nullptr, "input too short"); return nullptr; }
  }
  void *out = nullptr;
  napi_value out_v = nullptr;
  if (n_out) {
    const int64_t need = samples_needed(out_layout, h->S, n_out, out_pitch);
    if (need < 0) { napi_throw_range_error(env, nullptr, "output pitch too small"); return nullptr; }
    bool fresh = true;
    if (!(out_v = output_array(env, argc > 11, argv[11], sample_array_type(out_format), (size_t)need, fskhip_sample_bytes(out_format), &out, &fresh))) return nullptr;
    if (fresh) fill_silence(out_format, out, (size_t)need);
  }
  int rc = fskhip_processor_process_fmt_host(h->p, in, in_format, in_layout, n_in, in_pitch, out, out_format, out_layout, n_out, out_pitch, flags);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  if (!out_v) napi_get_null(env, &out_v);
  return out_v;
}

napi_value ProcessorModulate(napi_env env, napi_callback_info info) {
  ARGS(5);
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  void *pl, *lens, *mask; size_t plen, llen, mlen;
  if (!typed(env, argv[1], napi_uint8_array, &pl, &plen) || !typed(env, argv[2], napi_uint32_array, &lens, &llen) ||
      !typed(env, argv[4], napi_uint8_array, &mask, &mlen, true)) return nullptr;
  const uint32_t pitch = u32(env, argv[3]);
  if (llen < h->S || (size_t)pitch * h->S > plen || (mask && mlen < h->S)) { napi_throw_range_error(env, nullptr, "arguments too short"); return nullptr; }
  int rc = fskhip_processor_modulate_host(h->p, (const uint8_t *)pl, (const uint32_t *)lens, pitch, (const uint8_t *)mask);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

napi_value ProcessorTxState(napi_env env, napi_callback_info info) {
  ARGS(1);
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  void *pos, *total, *pending, *completed;
  napi_value pos_v = make_typed(env, napi_uint32_array, h->S, 4, &pos), tot_v = make_typed(env, napi_uint32_array, h->S, 4, &total);
  napi_value pen_v = make_typed(env, napi_uint8_array, h->S, 1, &pending), com_v = make_typed(env, napi_uint32_array, h->S, 4, &completed);
  int rc = fskhip_processor_tx_state_host(h->p, (uint32_t *)pos, (uint32_t *)total, (uint8_t *)pending, (uint32_t *)completed);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "pos", pos_v);
  napi_set_named_property(env, o, "total", tot_v);
  napi_set_named_property(env, o, "pending", pen_v);
  napi_set_named_property(env, o, "completed", com_v);
  return o;
}

napi_value ProcessorRxLength(napi_env env, napi_callback_info info) {
  ARGS(1);
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  void *lens;
  napi_value v = make_typed(env, napi_uint32_array, h->S, 4, &lens);
  int rc = fskhip_processor_rx_length_host(h->p, (uint32_t *)lens);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return v;
}

napi_value ProcessorLastTxKernel(napi_env env, napi_callback_info info) {
  ARGS(1);
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  napi_value v;
  napi_create_string_utf8(env, fskhip_processor_last_tx_kernel(h->p), NAPI_AUTO_LENGTH, &v);
  return v;
}

napi_value ProcessorDrain(napi_env env, napi_callback_info info) {
  ARGS(2);
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  const uint32_t cap = u32(env, argv[1]);
  void *out, *counts;
  napi_value out_v = make_typed(env, napi_uint8_array, (size_t)cap * h->S, 1, &out);
  napi_value cnt_v = make_typed(env, napi_uint32_array, h->S, 4, &counts);
  int rc = fskhip_processor_rx_drain_host(h->p, (uint8_t *)out, cap, (uint32_t *)counts);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "out", out_v);
  napi_set_named_property(env, o, "counts", cnt_v);
  set_u32(env, o, "outPitch", cap);
  return o;
}

// the compacted drain: sized with a query call (an overflowing call drains nothing), then drained into arrays of exactly that size
napi_value ProcessorDrainSparse(napi_env env, napi_callback_info info) {
  ARGS(3);
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  void *mask; size_t mlen;
  if (!typed(env, argv[1], napi_uint8_array, &mask, &mlen, true)) return nullptr;
  if (mask && mlen != h->S) { napi_throw_range_error(env, nullptr, "processorDrainSparse: mask must have one entry per stream"); return nullptr; }
  const uint32_t min_len = u32(env, argv[2]);
  uint32_t n_active = 0, n_bytes = 0;
  int rc = fskhip_processor_rx_drain_sparse_host(h->p, (const uint8_t *)mask, min_len, nullptr, nullptr, 0, nullptr, 0, &n_active, &n_bytes);
  if (rc != FSKHIP_OK && rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *streams, *offsets, *data;
  napi_value str_v = make_typed(env, napi_uint32_array, n_active, 4, &streams);
  napi_value off_v = make_typed(env, napi_uint32_array, (size_t)n_active + 1, 4, &offsets);
  napi_value dat_v = make_typed(env, napi_uint8_array, n_bytes, 1, &data);
  if (!str_v || !off_v || !dat_v) { napi_throw_error(env, nullptr, "processorDrainSparse: out of memory"); return nullptr; }
  if (rc == FSKHIP_E_OVERFLOW) {
    rc = fskhip_processor_rx_drain_sparse_host(h->p, (const uint8_t *)mask, min_len, (uint32_t *)streams, (uint32_t *)offsets, n_active, (uint8_t *)data,
                                               n_bytes, &n_active, &n_bytes);
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  } else {
    *(uint32_t *)offsets = 0u;
  }
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "streams", str_v);
  napi_set_named_property(env, o, "offsets", off_v);
  napi_set_named_property(env, o, "data", dat_v);
  return o;
}

napi_value ProcessorReset(napi_env env, napi_callback_info info) {
  ARGS(2);
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = fskhip_processor_reset(h->p, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// ---- the resident XModem receiver (include/fskhip_next.h: fskhip_xmodem_rx_*) over a processor handle.  The external owns a box, as
// the filters' do: close() empties it, and a receiver that is never closed is destroyed with its handle (destroy does not read the processor)
struct XmRx { fskhip_xmodem_rx *r; uint32_t S; };
void xm_rx_finalize(napi_env, void *data, void *) {
  XmRx *h = (XmRx *)data;
  if (h->r) fskhip_xmodem_rx_destroy(h->r);
  delete h;
}
XmRx *get_xm_rx(napi_env env, napi_value v) {
  XmRx *h = (XmRx *)external(env, v, "receiver destroyed");
  if (h && !h->r) { napi_throw_error(env, nullptr, "receiver destroyed"); return nullptr; }
  return h;
}
napi_value XmodemRxCreate(napi_env env, napi_callback_info info) {
  ARGS(1);
  Proc *p = get_proc(env, argv[0]);
  if (!p) return nullptr;
  fskhip_xmodem_rx *r = nullptr;
  int rc = fskhip_xmodem_rx_create(p->p, &r);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  XmRx *h = new XmRx{r, p->S};
  napi_value ext;
  if (napi_create_external(env, h, xm_rx_finalize, nullptr, &ext) != napi_ok) { xm_rx_finalize(env, h, nullptr); napi_throw_error(env, nullptr, "xmodemRxCreate: no handle"); return nullptr; }
  return ext;
}
napi_value XmodemRxDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  void *q = nullptr;
  if (napi_get_value_external(env, argv[0], &q) == napi_ok && q) {
    XmRx *h = (XmRx *)q;
    if (h->r) fskhip_xmodem_rx_destroy(h->r);
    h->r = nullptr;
  }
  return nullptr;
}
// sized with a query call (an overflowing poll changes nothing), then polled into arrays of exactly that size
napi_value XmodemRxPoll(napi_env env, napi_callback_info info) {
  ARGS(2);
  XmRx *h = get_xm_rx(env, argv[0]);
  if (!h) return nullptr;
  void *mask; size_t mlen;
  if (!typed(env, argv[1], napi_uint8_array, &mask, &mlen, true)) return nullptr;
  if (mask && mlen != h->S) { napi_throw_range_error(env, nullptr, "xmodemRxPoll: mask must have one entry per stream"); return nullptr; }
  uint32_t n_events = 0, n_bytes = 0;
  int rc = fskhip_xmodem_rx_poll_host(h->r, (const uint8_t *)mask, nullptr, nullptr, nullptr, 0, nullptr, 0, &n_events, &n_bytes);
  if (rc != FSKHIP_OK && rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *streams, *results, *offsets, *data;
  napi_value str_v = make_typed(env, napi_uint32_array, n_events, 4, &streams);
  napi_value res_v = make_typed(env, napi_int32_array, 10 * (size_t)n_events, 4, &results);
  napi_value off_v = make_typed(env, napi_uint32_array, (size_t)n_events + 1, 4, &offsets);
  napi_value dat_v = make_typed(env, napi_uint8_array, n_bytes, 1, &data);
  if (!str_v || !res_v || !off_v || !dat_v) { napi_throw_error(env, nullptr, "xmodemRxPoll: out of memory"); return nullptr; }
  if (rc == FSKHIP_E_OVERFLOW) {
    rc = fskhip_xmodem_rx_poll_host(h->r, (const uint8_t *)mask, (uint32_t *)streams, (fskhip_xmodem_result *)results, (uint32_t *)offsets, n_events,
                                    (uint8_t *)data, n_bytes, &n_events, &n_bytes);
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  } else {
    *(uint32_t *)offsets = 0u;
  }
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "streams", str_v);
  napi_set_named_property(env, o, "results", res_v);
  napi_set_named_property(env, o, "offsets", off_v);
  napi_set_named_property(env, o, "data", dat_v);
  return o;
}
napi_value XmodemRxReset(napi_env env, napi_callback_info info) {
  ARGS(2);
  XmRx *h = get_xm_rx(env, argv[0]);
  if (!h) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = fskhip_xmodem_rx_reset(h->r, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
napi_value XmodemRxState(napi_env env, napi_callback_info info) {
  ARGS(1);
  XmRx *h = get_xm_rx(env, argv[0]);
  if (!h) return nullptr;
  void *e, *p, *d;
  napi_value e_v = make_typed(env, napi_uint32_array, h->S, 4, &e), p_v = make_typed(env, napi_uint32_array, h->S, 4, &p);
  napi_value d_v = make_typed(env, napi_uint32_array, h->S, 4, &d);
  int rc = fskhip_xmodem_rx_state_get(h->r, (uint32_t *)e, (uint32_t *)p, (uint32_t *)d);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "expected", e_v);
  napi_set_named_property(env, o, "packets", p_v);
  napi_set_named_property(env, o, "dropped", d_v);
  return o;
}
napi_value XmodemRxSetState(napi_env env, napi_callback_info info) {
  ARGS(4);
  XmRx *h = get_xm_rx(env, argv[0]);
  if (!h) return nullptr;
  void *a[3]; size_t n[3];
  for (int i = 0; i < 3; i++) {
    if (!typed(env, argv[1 + i], napi_uint32_array, &a[i], &n[i], true)) return nullptr;
    if (a[i] && n[i] != h->S) { napi_throw_range_error(env, nullptr, "xmodemRxSetState: state arrays must have one entry per stream"); return nullptr; }
  }
  int rc = fskhip_xmodem_rx_state_set(h->r, (const uint32_t *)a[0], (const uint32_t *)a[1], (const uint32_t *)a[2]);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// ---- the resident XModem sender (include/fskhip_next.h: fskhip_xmodem_tx_*) over a processor handle, boxed as the receiver is
struct XmTx { fskhip_xmodem_tx *t; uint32_t S; };
void xm_tx_finalize(napi_env, void *data, void *) {
  XmTx *h = (XmTx *)data;
  if (h->t) fskhip_xmodem_tx_destroy(h->t);
  delete h;
}
XmTx *get_xm_tx(napi_env env, napi_value v) {
  XmTx *h = (XmTx *)external(env, v, "sender destroyed");
  if (h && !h->t) { napi_throw_error(env, nullptr, "sender destroyed"); return nullptr; }
  return h;
}
napi_value XmodemTxCreate(napi_env env, napi_callback_info info) {
  ARGS(3);
  Proc *p = get_proc(env, argv[0]);
  if (!p) return nullptr;
  uint32_t max_payload = 0, max_retries = 0;
  napi_get_value_uint32(env, argv[1], &max_payload);
  napi_get_value_uint32(env, argv[2], &max_retries);
  fskhip_xmodem_tx *t = nullptr;
  int rc = fskhip_xmodem_tx_create(p->p, max_payload, max_retries, &t);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  XmTx *h = new XmTx{t, p->S};
  napi_value ext;
  if (napi_create_external(env, h, xm_tx_finalize, nullptr, &ext) != napi_ok) { xm_tx_finalize(env, h, nullptr); napi_throw_error(env, nullptr, "xmodemTxCreate: no handle"); return nullptr; }
  return ext;
}
napi_value XmodemTxDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  void *q = nullptr;
  if (napi_get_value_external(env, argv[0], &q) == napi_ok && q) {
    XmTx *h = (XmTx *)q;
    if (h->t) fskhip_xmodem_tx_destroy(h->t);
    h->t = nullptr;
  }
  return nullptr;
}
napi_value XmodemTxSend(napi_env env, napi_callback_info info) {
  ARGS(4);
  XmTx *h = get_xm_tx(env, argv[0]);
  if (!h) return nullptr;
  void *mask, *off, *data; size_t mlen, olen, dlen;
  if (!typed(env, argv[1], napi_uint8_array, &mask, &mlen, true) || !typed(env, argv[2], napi_uint32_array, &off, &olen) ||
      !typed(env, argv[3], napi_uint8_array, &data, &dlen))
    return nullptr;
  if (mask && mlen != h->S) { napi_throw_range_error(env, nullptr, "xmodemTxSend: mask must have one entry per stream"); return nullptr; }
  if (olen != (size_t)h->S + 1) { napi_throw_range_error(env, nullptr, "xmodemTxSend: offsets must have nStreams + 1 entries"); return nullptr; }
  std::vector<uint64_t> offsets(olen);
  for (size_t i = 0; i < olen; i++) {
    offsets[i] = ((const uint32_t *)off)[i];
    if (offsets[i] > dlen) { napi_throw_range_error(env, nullptr, "xmodemTxSend: an offset lies behind the data"); return nullptr; }
  }
  int rc = fskhip_xmodem_tx_send_host(h->t, (const uint8_t *)mask, offsets.data(), (const uint8_t *)data);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
// sized with a query call (an overflowing poll changes nothing), then polled into arrays of exactly that size
napi_value XmodemTxPoll(napi_env env, napi_callback_info info) {
  ARGS(3);
  XmTx *h = get_xm_tx(env, argv[0]);
  if (!h) return nullptr;
  void *mask, *abort_; size_t mlen, alen;
  if (!typed(env, argv[1], napi_uint8_array, &mask, &mlen, true) || !typed(env, argv[2], napi_uint8_array, &abort_, &alen, true)) return nullptr;
  if ((mask && mlen != h->S) || (abort_ && alen != h->S)) { napi_throw_range_error(env, nullptr, "xmodemTxPoll: mask and abort must have one entry per stream"); return nullptr; }
  uint32_t n_events = 0;
  int rc = fskhip_xmodem_tx_poll_host(h->t, (const uint8_t *)mask, (const uint8_t *)abort_, nullptr, nullptr, 0, &n_events);
  if (rc != FSKHIP_OK && rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *streams, *events;
  napi_value str_v = make_typed(env, napi_uint32_array, n_events, 4, &streams);
  napi_value ev_v = make_typed(env, napi_int32_array, 8 * (size_t)n_events, 4, &events);
  if (!str_v || !ev_v) { napi_throw_error(env, nullptr, "xmodemTxPoll: out of memory"); return nullptr; }
  if (rc == FSKHIP_E_OVERFLOW) {
    rc = fskhip_xmodem_tx_poll_host(h->t, (const uint8_t *)mask, (const uint8_t *)abort_, (uint32_t *)streams, (fskhip_xmodem_tx_event *)events, n_events, &n_events);
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  }
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "streams", str_v);
  napi_set_named_property(env, o, "events", ev_v);
  return o;
}
napi_value XmodemTxReset(napi_env env, napi_callback_info info) {
  ARGS(2);
  XmTx *h = get_xm_tx(env, argv[0]);
  if (!h) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = fskhip_xmodem_tx_reset(h->t, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
const char *const kXmTxWords[6] = {"state", "sequence", "fragmentIndex", "retries", "packetsSent", "retransmitted"};
napi_value XmodemTxState(napi_env env, napi_callback_info info) {
  ARGS(1);
  XmTx *h = get_xm_tx(env, argv[0]);
  if (!h) return nullptr;
  void *a[6]; napi_value v[6];
  for (int i = 0; i < 6; i++) {
    v[i] = make_typed(env, napi_uint32_array, h->S, 4, &a[i]);
    if (!v[i]) { napi_throw_error(env, nullptr, "xmodemTxState: out of memory"); return nullptr; }
  }
  int rc = fskhip_xmodem_tx_state_get(h->t, (uint32_t *)a[0], (uint32_t *)a[1], (uint32_t *)a[2], (uint32_t *)a[3], (uint32_t *)a[4], (uint32_t *)a[5]);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  for (int i = 0; i < 6; i++) napi_set_named_property(env, o, kXmTxWords[i], v[i]);
  return o;
}
napi_value XmodemTxSetState(napi_env env, napi_callback_info info) {
  ARGS(7);
  XmTx *h = get_xm_tx(env, argv[0]);
  if (!h) return nullptr;
  void *a[6]; size_t n[6];
  for (int i = 0; i < 6; i++) {
    if (!typed(env, argv[1 + i], napi_uint32_array, &a[i], &n[i], true)) return nullptr;
    if (a[i] && n[i] != h->S) { napi_throw_range_error(env, nullptr, "xmodemTxSetState: state arrays must have one entry per stream"); return nullptr; }
  }
  int rc = fskhip_xmodem_tx_state_set(h->t, (const uint32_t *)a[0], (const uint32_t *)a[1], (const uint32_t *)a[2], (const uint32_t *)a[3], (const uint32_t *)a[4],
                                      (const uint32_t *)a[5]);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// ---- the resident XModem file receiver (include/fskhip_next.h: fskhip_xmodem_recv_*) over a processor handle, boxed as the sender is
struct XmRecv { fskhip_xmodem_recv *r; uint32_t S; };
void xm_recv_finalize(napi_env, void *data, void *) {
  XmRecv *h = (XmRecv *)data;
  if (h->r) fskhip_xmodem_recv_destroy(h->r);
  delete h;
}
XmRecv *get_xm_recv(napi_env env, napi_value v) {
  XmRecv *h = (XmRecv *)external(env, v, "receiver destroyed");
  if (h && !h->r) { napi_throw_error(env, nullptr, "receiver destroyed"); return nullptr; }
  return h;
}
napi_value XmodemRecvCreate(napi_env env, napi_callback_info info) {
  ARGS(3);
  Proc *p = get_proc(env, argv[0]);
  if (!p) return nullptr;
  uint32_t file_capacity = 0, max_retries = 0;
  napi_get_value_uint32(env, argv[1], &file_capacity);
  napi_get_value_uint32(env, argv[2], &max_retries);
  fskhip_xmodem_recv *r = nullptr;
  int rc = fskhip_xmodem_recv_create(p->p, file_capacity, max_retries, &r);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  XmRecv *h = new XmRecv{r, p->S};
  napi_value ext;
  if (napi_create_external(env, h, xm_recv_finalize, nullptr, &ext) != napi_ok) { xm_recv_finalize(env, h, nullptr); napi_throw_error(env, nullptr, "xmodemRecvCreate: no handle"); return nullptr; }
  return ext;
}
napi_value XmodemRecvDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  void *q = nullptr;
  if (napi_get_value_external(env, argv[0], &q) == napi_ok && q) {
    XmRecv *h = (XmRecv *)q;
    if (h->r) fskhip_xmodem_recv_destroy(h->r);
    h->r = nullptr;
  }
  return nullptr;
}
napi_value XmodemRecvStart(napi_env env, napi_callback_info info) {
  ARGS(2);
  XmRecv *h = get_xm_recv(env, argv[0]);
  if (!h) return nullptr;
  void *mask; size_t mlen;
  if (!typed(env, argv[1], napi_uint8_array, &mask, &mlen, true)) return nullptr;
  if (mask && mlen != h->S) { napi_throw_range_error(env, nullptr, "xmodemRecvStart: mask must have one entry per stream"); return nullptr; }
  int rc = fskhip_xmodem_recv_start_host(h->r, (const uint8_t *)mask);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
// sized with a query call (an overflowing poll changes nothing), then polled into arrays of exactly that size
napi_value XmodemRecvPoll(napi_env env, napi_callback_info info) {
  ARGS(4);
  XmRecv *h = get_xm_recv(env, argv[0]);
  if (!h) return nullptr;
  void *m[3]; size_t len[3];
  for (int i = 0; i < 3; i++) {
    if (!typed(env, argv[1 + i], napi_uint8_array, &m[i], &len[i], true)) return nullptr;
    if (m[i] && len[i] != h->S) { napi_throw_range_error(env, nullptr, "xmodemRecvPoll: mask, timeout and abort must have one entry per stream"); return nullptr; }
  }
  uint32_t n_events = 0;
  int rc = fskhip_xmodem_recv_poll_host(h->r, (const uint8_t *)m[0], (const uint8_t *)m[1], (const uint8_t *)m[2], nullptr, nullptr, 0, &n_events);
  if (rc != FSKHIP_OK && rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *streams, *events;
  napi_value str_v = make_typed(env, napi_uint32_array, n_events, 4, &streams);
  napi_value ev_v = make_typed(env, napi_int32_array, 12 * (size_t)n_events, 4, &events);
  if (!str_v || !ev_v) { napi_throw_error(env, nullptr, "xmodemRecvPoll: out of memory"); return nullptr; }
  if (rc == FSKHIP_E_OVERFLOW) {
    rc = fskhip_xmodem_recv_poll_host(h->r, (const uint8_t *)m[0], (const uint8_t *)m[1], (const uint8_t *)m[2], (uint32_t *)streams, (fskhip_xmodem_recv_event *)events,
                                      n_events, &n_events);
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  }
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "streams", str_v);
  napi_set_named_property(env, o, "events", ev_v);
  return o;
}
napi_value XmodemRecvReset(napi_env env, napi_callback_info info) {
  ARGS(2);
  XmRecv *h = get_xm_recv(env, argv[0]);
  if (!h) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = fskhip_xmodem_recv_reset(h->r, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
// sized with a query call (a cap that is too small copies nothing), then read into an array of exactly that size
napi_value XmodemRecvFiles(napi_env env, napi_callback_info info) {
  ARGS(2);
  XmRecv *h = get_xm_recv(env, argv[0]);
  if (!h) return nullptr;
  void *sel; size_t n_sel;
  if (!typed(env, argv[1], napi_uint32_array, &sel, &n_sel)) return nullptr;
  if (n_sel > 0xFFFFFFFFull) { napi_throw_range_error(env, nullptr, "xmodemRecvFiles: too many streams"); return nullptr; }
  std::vector<uint64_t> offsets(n_sel + 1, 0u);
  uint64_t n_bytes = 0;
  int rc = fskhip_xmodem_recv_files_host(h->r, (const uint32_t *)sel, (uint32_t)n_sel, offsets.data(), nullptr, 0, &n_bytes);
  if (rc != FSKHIP_OK && rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *data, *off;
  napi_value data_v = make_typed(env, napi_uint8_array, (size_t)n_bytes, 1, &data);
  napi_value off_v = make_typed(env, napi_float64_array, n_sel + 1, 8, &off);
  if (!data_v || !off_v) { napi_throw_error(env, nullptr, "xmodemRecvFiles: out of memory"); return nullptr; }
  if (rc == FSKHIP_E_OVERFLOW) {
    rc = fskhip_xmodem_recv_files_host(h->r, (const uint32_t *)sel, (uint32_t)n_sel, offsets.data(), (uint8_t *)data, (size_t)n_bytes, &n_bytes);
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  }
  for (size_t i = 0; i <= n_sel; i++) ((double *)off)[i] = (double)offsets[i];
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "offsets", off_v);
  napi_set_named_property(env, o, "data", data_v);
  return o;
}
napi_value XmodemRecvSetFiles(napi_env env, napi_callback_info info) {
  ARGS(4);
  XmRecv *h = get_xm_recv(env, argv[0]);
  if (!h) return nullptr;
  void *sel, *off, *data; size_t n_sel, olen, dlen;
  if (!typed(env, argv[1], napi_uint32_array, &sel, &n_sel) || !typed(env, argv[2], napi_uint32_array, &off, &olen) || !typed(env, argv[3], napi_uint8_array, &data, &dlen))
    return nullptr;
  if (olen != n_sel + 1 || n_sel > 0xFFFFFFFFull) { napi_throw_range_error(env, nullptr, "xmodemRecvSetFiles: offsets must have one entry per selected stream and one more"); return nullptr; }
  std::vector<uint64_t> offsets(olen);
  for (size_t i = 0; i < olen; i++) {
    offsets[i] = ((const uint32_t *)off)[i];
    if (offsets[i] > dlen) { napi_throw_range_error(env, nullptr, "xmodemRecvSetFiles: an offset lies behind the data"); return nullptr; }
  }
  int rc = fskhip_xmodem_recv_files_set_host(h->r, (const uint32_t *)sel, (uint32_t)n_sel, offsets.data(), (const uint8_t *)data);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
const char *const kXmRecvWords[7] = {"state", "expected", "retries", "fileLen", "packetsReceived", "dropped", "packetsSent"};
napi_value XmodemRecvState(napi_env env, napi_callback_info info) {
  ARGS(1);
  XmRecv *h = get_xm_recv(env, argv[0]);
  if (!h) return nullptr;
  void *a[7]; napi_value v[7];
  for (int i = 0; i < 7; i++) {
    v[i] = make_typed(env, napi_uint32_array, h->S, 4, &a[i]);
    if (!v[i]) { napi_throw_error(env, nullptr, "xmodemRecvState: out of memory"); return nullptr; }
  }
  int rc = fskhip_xmodem_recv_state_get(h->r, (uint32_t *)a[0], (uint32_t *)a[1], (uint32_t *)a[2], (uint32_t *)a[3], (uint32_t *)a[4], (uint32_t *)a[5], (uint32_t *)a[6]);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  for (int i = 0; i < 7; i++) napi_set_named_property(env, o, kXmRecvWords[i], v[i]);
  return o;
}
napi_value XmodemRecvSetState(napi_env env, napi_callback_info info) {
  ARGS(8);
  XmRecv *h = get_xm_recv(env, argv[0]);
  if (!h) return nullptr;
  void *a[7]; size_t n[7];
  for (int i = 0; i < 7; i++) {
    if (!typed(env, argv[1 + i], napi_uint32_array, &a[i], &n[i], true)) return nullptr;
    if (a[i] && n[i] != h->S) { napi_throw_range_error(env, nullptr, "xmodemRecvSetState: state arrays must have one entry per stream"); return nullptr; }
  }
  int rc = fskhip_xmodem_recv_state_set(h->r, (const uint32_t *)a[0], (const uint32_t *)a[1], (const uint32_t *)a[2], (const uint32_t *)a[3], (const uint32_t *)a[4],
                                        (const uint32_t *)a[5], (const uint32_t *)a[6]);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// ---- the resident XModem wait timers (include/fskhip_next.h: fskhip_xmodem_timer_*) over a file receiver's or a sender's handle
struct XmTimer { fskhip_xmodem_timer *w; uint32_t S; bool recv; };
void xm_timer_finalize(napi_env, void *data, void *) {
  XmTimer *h = (XmTimer *)data;
  if (h->w) fskhip_xmodem_timer_destroy(h->w);
  delete h;
}
XmTimer *get_xm_timer(napi_env env, napi_value v) {
  XmTimer *h = (XmTimer *)external(env, v, "timers destroyed");
  if (h && !h->w) { napi_throw_error(env, nullptr, "timers destroyed"); return nullptr; }
  return h;
}
napi_value XmodemTimerCreate(napi_env env, napi_callback_info info) {
  ARGS(3);
  bool recv = false;
  napi_get_value_bool(env, argv[0], &recv);
  uint32_t timeout_samples = 0, S = 0;
  napi_get_value_uint32(env, argv[2], &timeout_samples);
  fskhip_xmodem_timer *w = nullptr;
  int rc;
  if (recv) {
    XmRecv *r = get_xm_recv(env, argv[1]);
    if (!r) return nullptr;
    S = r->S;
    rc = fskhip_xmodem_timer_create_recv(r->r, timeout_samples, &w);
  } else {
    XmTx *t = get_xm_tx(env, argv[1]);
    if (!t) return nullptr;
    S = t->S;
    rc = fskhip_xmodem_timer_create_tx(t->t, timeout_samples, &w);
  }
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  XmTimer *h = new XmTimer{w, S, recv};
  napi_value ext;
  if (napi_create_external(env, h, xm_timer_finalize, nullptr, &ext) != napi_ok) { xm_timer_finalize(env, h, nullptr); napi_throw_error(env, nullptr, "xmodemTimerCreate: no handle"); return nullptr; }
  return ext;
}
napi_value XmodemTimerDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  void *q = nullptr;
  if (napi_get_value_external(env, argv[0], &q) == napi_ok && q) {
    XmTimer *h = (XmTimer *)q;
    if (h->w) fskhip_xmodem_timer_destroy(h->w);
    h->w = nullptr;
  }
  return nullptr;
}
// sized with a query call (an overflowing timed poll changes nothing, the timers included), then polled into arrays of exactly that size
napi_value XmodemTimerPoll(napi_env env, napi_callback_info info) {
  ARGS(4);
  XmTimer *h = get_xm_timer(env, argv[0]);
  if (!h) return nullptr;
  uint32_t elapsed = 0;
  napi_get_value_uint32(env, argv[1], &elapsed);
  void *mask, *abort_; size_t mlen, alen;
  if (!typed(env, argv[2], napi_uint8_array, &mask, &mlen, true) || !typed(env, argv[3], napi_uint8_array, &abort_, &alen, true)) return nullptr;
  if ((mask && mlen != h->S) || (abort_ && alen != h->S)) { napi_throw_range_error(env, nullptr, "xmodemTimerPoll: mask and abort must have one entry per stream"); return nullptr; }
  const size_t words = h->recv ? 12 : 8;
  auto poll = [&](void *streams, void *events, uint32_t cap, uint32_t *n_events) {
    return h->recv ? fskhip_xmodem_recv_poll_timed_host(h->w, elapsed, (const uint8_t *)mask, (const uint8_t *)abort_, (uint32_t *)streams, (fskhip_xmodem_recv_event *)events, cap, n_events)
                   : fskhip_xmodem_tx_poll_timed_host(h->w, elapsed, (const uint8_t *)mask, (const uint8_t *)abort_, (uint32_t *)streams, (fskhip_xmodem_tx_event *)events, cap, n_events);
  };
  uint32_t n_events = 0;
  int rc = poll(nullptr, nullptr, 0, &n_events);
  if (rc != FSKHIP_OK && rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *streams, *events;
  napi_value str_v = make_typed(env, napi_uint32_array, n_events, 4, &streams);
  napi_value ev_v = make_typed(env, napi_int32_array, words * (size_t)n_events, 4, &events);
  if (!str_v || !ev_v) { napi_throw_error(env, nullptr, "xmodemTimerPoll: out of memory"); return nullptr; }
  if (rc == FSKHIP_E_OVERFLOW) {
    rc = poll(streams, events, n_events, &n_events);
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  }
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "streams", str_v);
  napi_set_named_property(env, o, "events", ev_v);
  return o;
}
napi_value XmodemTimerReset(napi_env env, napi_callback_info info) {
  ARGS(2);
  XmTimer *h = get_xm_timer(env, argv[0]);
  if (!h) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = fskhip_xmodem_timer_reset(h->w, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
napi_value XmodemTimerState(napi_env env, napi_callback_info info) {
  ARGS(1);
  XmTimer *h = get_xm_timer(env, argv[0]);
  if (!h) return nullptr;
  void *a[2]; napi_value v[2];
  for (int i = 0; i < 2; i++) {
    v[i] = make_typed(env, napi_uint32_array, h->S, 4, &a[i]);
    if (!v[i]) { napi_throw_error(env, nullptr, "xmodemTimerState: out of memory"); return nullptr; }
  }
  int rc = fskhip_xmodem_timer_state_get(h->w, (uint32_t *)a[0], (uint32_t *)a[1]);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  napi_set_named_property(env, o, "waited", v[0]);
  napi_set_named_property(env, o, "mark", v[1]);
  return o;
}
napi_value XmodemTimerSetState(napi_env env, napi_callback_info info) {
  ARGS(3);
  XmTimer *h = get_xm_timer(env, argv[0]);
  if (!h) return nullptr;
  void *a[2]; size_t n[2];
  for (int i = 0; i < 2; i++) {
    if (!typed(env, argv[1 + i], napi_uint32_array, &a[i], &n[i], true)) return nullptr;
    if (a[i] && n[i] != h->S) { napi_throw_range_error(env, nullptr, "xmodemTimerSetState: state arrays must have one entry per stream"); return nullptr; }
  }
  int rc = fskhip_xmodem_timer_state_set(h->w, (const uint32_t *)a[0], (const uint32_t *)a[1]);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// ---- processor remap / snapshots (include/fskhip_next.h): a snapshot is a Buffer (or any Uint8Array) on this side
napi_value ProcessorRemap(napi_env env, napi_callback_info info) {
  ARGS(3);
  Proc *dst = get_proc(env, argv[0]);
  if (!dst) return nullptr;
  Proc *src = get_proc(env, argv[1]);
  if (!src) return nullptr;
  std::vector<int64_t> map;
  if (!index_array(env, argv[2], "processorRemap: map must be an Array of integer stream indices (-1: a new stream)", &map)) return nullptr;
  int rc = fskhip_processor_remap(dst->p, src->p, index_data(map), (uint32_t)map.size());
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

napi_value ProcessorSnapshot(napi_env env, napi_callback_info info) {
  ARGS(2);
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  std::vector<int64_t> sel;
  const bool all = nullish(env, argv[1]);
  if (!all && !index_array(env, argv[1], "processorSnapshot: sel must be an Array of integer stream indices", &sel)) return nullptr;
  const int64_t *sp = index_data(sel, all);
  const uint32_t n = all ? h->S : (uint32_t)sel.size();
  size_t need = 0;
  int rc = fskhip_processor_snapshot(h->p, sp, n, nullptr, 0, &need);   // (the size: it depends on the pending payloads)
  if (rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *data = nullptr;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, need, &data, &buf));
  rc = fskhip_processor_snapshot(h->p, sp, n, data, need, nullptr);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return buf;
}

napi_value ProcessorRestore(napi_env env, napi_callback_info info) {
  ARGS(3);
  Proc *dst = get_proc(env, argv[0]);
  if (!dst) return nullptr;
  void *data; size_t size;
  if (!typed(env, argv[1], napi_uint8_array, &data, &size)) return nullptr;
  std::vector<int64_t> map;
  if (!index_array(env, argv[2], "processorRestore: map must be an Array of integer record indices (-1: a new stream)", &map)) return nullptr;
  int rc = fskhip_processor_restore(dst->p, data, size, index_data(map), (uint32_t)map.size());
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// processorSnapshotConcat([image, ...]) -> Buffer: the records of all of them under one header, in canonical form (host only)
napi_value ProcessorSnapshotConcat(napi_env env, napi_callback_info info) {
  ARGS(1);
  bool is_arr = false;
  if (napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) { napi_throw_type_error(env, nullptr, "processorSnapshotConcat: an Array of processor snapshots"); return nullptr; }
  uint32_t n = 0;
  NAPI_OK(napi_get_array_length(env, argv[0], &n));
  std::vector<const void *> ptrs(n);
  std::vector<size_t> sizes(n);
  for (uint32_t k = 0; k < n; k++) {
    napi_value v;
    void *data;
    NAPI_OK(napi_get_element(env, argv[0], k, &v));
    if (!typed(env, v, napi_uint8_array, &data, &sizes[k])) return nullptr;
    ptrs[k] = data;
  }
  size_t need = 0;
  int rc = fskhip_processor_snapshot_concat(ptrs.data(), sizes.data(), n, nullptr, 0, &need);
  if (rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *data = nullptr;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, need, &data, &buf));
  rc = fskhip_processor_snapshot_concat(ptrs.data(), sizes.data(), n, data, need, nullptr);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return buf;
}

napi_value ProcessorSnapshotInfo(napi_env env, napi_callback_info info) {
  ARGS(1);
  void *data; size_t size;
  if (!typed(env, argv[0], napi_uint8_array, &data, &size)) return nullptr;
  fskhip_processor_snapshot_info si;
  int rc = fskhip_processor_snapshot_info_get(data, size, &si);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  set_u32(env, o, "nStreams", si.n_streams);
  set_u32(env, o, "rxCapacity", si.rx_capacity);
  set_u32(env, o, "payloadCapacity", si.payload_capacity);
  set_u32(env, o, "recordBytes", si.record_bytes);
  return o;
}

// ---- the resident XModem handles through remap / snapshot / restore (include/fskhip_next.h): one spelling for the three kinds
#define XM_LIFECYCLE(Name, Box, get, field, kind)                                                                                   \
  napi_value Xmodem##Name##Remap(napi_env env, napi_callback_info info) {                                                            \
    ARGS(3);                                                                                                                         \
    Box *dst = get(env, argv[0]);                                                                                                    \
    if (!dst) return nullptr;                                                                                                        \
    Box *src = get(env, argv[1]);                                                                                                    \
    if (!src) return nullptr;                                                                                                        \
    std::vector<int64_t> map;                                                                                                        \
    if (!index_array(env, argv[2], "xmodem" #Name "Remap: map must be an Array of integer stream indices (-1: a new stream)", &map)) return nullptr; \
    int rc = fskhip_xmodem_##kind##_remap(dst->field, src->field, index_data(map), (uint32_t)map.size());                            \
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);                                                                                  \
    return nullptr;                                                                                                                  \
  }                                                                                                                                  \
  napi_value Xmodem##Name##Snapshot(napi_env env, napi_callback_info info) {                                                         \
    ARGS(2);                                                                                                                         \
    Box *h = get(env, argv[0]);                                                                                                      \
    if (!h) return nullptr;                                                                                                          \
    std::vector<int64_t> sel;                                                                                                        \
    const bool all = nullish(env, argv[1]);                                                                                          \
    if (!all && !index_array(env, argv[1], "xmodem" #Name "Snapshot: sel must be an Array of integer stream indices", &sel)) return nullptr; \
    const int64_t *sp = index_data(sel, all);                                                                                        \
    const uint32_t n = all ? h->S : (uint32_t)sel.size();                                                                            \
    size_t need = 0;                                                                                                                 \
    int rc = fskhip_xmodem_##kind##_snapshot(h->field, sp, n, nullptr, 0, &need);   /* (the size: it depends on the files) */        \
    if (rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);                                                                          \
    void *data = nullptr;                                                                                                            \
    napi_value buf;                                                                                                                  \
    NAPI_OK(napi_create_buffer(env, need, &data, &buf));                                                                             \
    rc = fskhip_xmodem_##kind##_snapshot(h->field, sp, n, data, need, nullptr);                                                      \
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);                                                                                  \
    return buf;                                                                                                                      \
  }                                                                                                                                  \
  napi_value Xmodem##Name##Restore(napi_env env, napi_callback_info info) {                                                          \
    ARGS(3);                                                                                                                         \
    Box *dst = nullish(env, argv[0]) ? nullptr : get(env, argv[0]);                                                                  \
    if (!dst && !nullish(env, argv[0])) return nullptr;                                                                              \
    void *data; size_t size;                                                                                                         \
    if (!typed(env, argv[1], napi_uint8_array, &data, &size)) return nullptr;                                                        \
    std::vector<int64_t> map;                                                                                                        \
    if (!index_array(env, argv[2], "xmodem" #Name "Restore: map must be an Array of integer record indices (-1: a new stream)", &map)) return nullptr; \
    int rc = fskhip_xmodem_##kind##_restore(dst ? dst->field : nullptr, data, size, index_data(map), (uint32_t)map.size());          \
    if (rc != FSKHIP_OK) return throw_fsk(env, rc);                                                                                  \
    return nullptr;                                                                                                                  \
  }
XM_LIFECYCLE(Rx, XmRx, get_xm_rx, r, rx)
XM_LIFECYCLE(Tx, XmTx, get_xm_tx, t, tx)
XM_LIFECYCLE(Recv, XmRecv, get_xm_recv, r, recv)
XM_LIFECYCLE(Timer, XmTimer, get_xm_timer, w, timer)   // the wait timers' two words, with the map their handle was carried with
#undef XM_LIFECYCLE

napi_value XmodemSnapshotInfo(napi_env env, napi_callback_info info) {
  ARGS(1);
  void *data; size_t size;
  if (!typed(env, argv[0], napi_uint8_array, &data, &size)) return nullptr;
  fskhip_xmodem_snapshot_info si;
  int rc = fskhip_xmodem_snapshot_info_get(data, size, &si);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  set_u32(env, o, "kind", si.kind);
  set_u32(env, o, "nStreams", si.n_streams);
  set_u32(env, o, "param0", si.param0);
  set_u32(env, o, "param1", si.param1);
  set_num(env, o, "fileBytes", (double)si.file_bytes);
  return o;
}

napi_value XmodemTimerSnapshotInfo(napi_env env, napi_callback_info info) {
  ARGS(1);
  void *data; size_t size;
  if (!typed(env, argv[0], napi_uint8_array, &data, &size)) return nullptr;
  fskhip_xmodem_timer_snapshot_info si;
  int rc = fskhip_xmodem_timer_snapshot_info_get(data, size, &si);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  set_u32(env, o, "kind", si.kind);
  set_u32(env, o, "nStreams", si.n_streams);
  set_u32(env, o, "timeoutSamples", si.timeout_samples);
  return o;
}

// ---- FIR ------------------------------------------------------------------------------------------------
napi_value sinc_result(napi_env env, int n, const std::vector<double> &t) {
  if (n < 0) return throw_fsk(env, n);
  void *out;
  napi_value v = make_typed(env, napi_float64_array, (size_t)n, 8, &out);
  memcpy(out, t.data(), sizeof(double) * (size_t)n);
  return v;
}
napi_value SincLowpass(napi_env env, napi_callback_info info) {
  ARGS(3);
  const uint32_t nt = u32(env, argv[2]);
  std::vector<double> t(nt + 2);
  return sinc_result(env, fskhip_sinc_lowpass(f64(env, argv[0]), f64(env, argv[1]), nt, t.data()), t);
}
napi_value SincHighpass(napi_env env, napi_callback_info info) {
  ARGS(3);
  const uint32_t nt = u32(env, argv[2]);
  std::vector<double> t(nt + 2);
  return sinc_result(env, fskhip_sinc_highpass(f64(env, argv[0]), f64(env, argv[1]), nt, t.data()), t);
}
napi_value SincBandpass(napi_env env, napi_callback_info info) {
  ARGS(4);
  const uint32_t nt = u32(env, argv[3]);
  std::vector<double> t(nt + 2);
  return sinc_result(env, fskhip_sinc_bandpass(f64(env, argv[0]), f64(env, argv[1]), f64(env, argv[2]), nt, t.data()), t);
}

napi_value FirCreate(napi_env env, napi_callback_info info) {
  ARGS(4);
  void *taps; size_t nt;
  if (!typed(env, argv[0], napi_float64_array, &taps, &nt)) return nullptr;
  fskhip_fir *f = nullptr;
  int rc = fskhip_fir_create(i32(env, argv[2]), (const double *)taps, (uint32_t)nt, u32(env, argv[1]), i32(env, argv[3]), &f);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return filter_box_new(env, f, BOX_FIR);
}
napi_value FirDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  filter_box_close(env, argv[0]);
  return nullptr;
}
napi_value FirProcess(napi_env env, napi_callback_info info) {
  ARGS(5);
  fskhip_fir *f = (fskhip_fir *)filter_of(env, argv[0]);
  if (!f) return nullptr;
  void *in; size_t ilen;
  if (!typed(env, argv[1], napi_float32_array, &in, &ilen)) return nullptr;
  const uint32_t n = u32(env, argv[2]), pitch = u32(env, argv[3]), S = u32(env, argv[4]);
  if (S != fskhip_fir_streams(f)) { napi_throw_range_error(env, nullptr, "nStreams is not the filter's stream count"); return nullptr; }
  if (S == 0 || pitch < n || (size_t)pitch * (S - 1) + n > ilen) { napi_throw_range_error(env, nullptr, "input too short"); return nullptr; }
  void *out;
  napi_value out_v = make_typed(env, napi_float32_array, (size_t)n * S, 4, &out);
  int rc = fskhip_fir_process_host(f, (const float *)in, n, pitch, (float *)out, n);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return out_v;
}
napi_value FirReset(napi_env env, napi_callback_info info) {
  ARGS(2);
  fskhip_fir *f = (fskhip_fir *)filter_of(env, argv[0]);
  if (!f) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = fskhip_fir_reset(f, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// ---- resampler (include/fskhip_next.h: fskhip_resampler_*) ----
napi_value ResamplerCreate(napi_env env, napi_callback_info info) {   // (direction, factor, taps: Float64Array, nStreams, device, precision)
  ARGS(6);
  void *taps; size_t nt;
  if (!typed(env, argv[2], napi_float64_array, &taps, &nt)) return nullptr;
  fskhip_resampler *r = nullptr;
  int rc = fskhip_resampler_create(i32(env, argv[4]), i32(env, argv[0]), u32(env, argv[1]), (const double *)taps, (uint32_t)nt, u32(env, argv[3]),
                                   i32(env, argv[5]), &r);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return filter_box_new(env, r, BOX_RESAMPLER);
}
napi_value ResamplerDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  filter_box_close(env, argv[0]);
  return nullptr;
}
// The calls the resampler shares with the rate converter below (fskhip_ratecvt_*), each body once over the unit's C entry points.
// by_factor: the last argument of the two process calls is the factor, as the resampler's take it, else the output count.
template <class H>
struct RateApi {
  H *(*of)(napi_env, napi_value);
  uint32_t (*streams)(const H *), (*history)(const H *);
  int (*reset)(H *, int64_t), (*state_get)(H *, float *), (*state_set)(H *, const float *);
  int (*widen)(H *, const void *, int, int, size_t, size_t, float *, size_t);
  int (*narrow)(H *, const float *, size_t, size_t, const uint32_t *, void *, int, int, size_t);
  bool by_factor;
};
template <class H>
napi_value rate_count(napi_env env, napi_callback_info info, const RateApi<H> &A, uint32_t (*count)(const H *)) {
  ARGS(1);
  H *r = A.of(env, argv[0]);
  if (!r) return nullptr;
  napi_value v;
  NAPI_OK(napi_create_uint32(env, count(r), &v));
  return v;
}
// (handle, samples in the format's typed array, format, layout, nIn, pitch, factor | nOut) -> Float32Array [S][nOut]
template <class H>
napi_value rate_widen(napi_env env, napi_callback_info info, const RateApi<H> &A) {
  ARGS(7);
  const int32_t format = i32(env, argv[2]), layout = i32(env, argv[3]);
  if (!sample_format_ok(env, format, layout)) return nullptr;
  H *r = A.of(env, argv[0]);
  if (!r) return nullptr;
  void *in; size_t ilen;
  if (!typed(env, argv[1], sample_array_type(format), &in, &ilen)) return nullptr;
  const uint32_t n = u32(env, argv[4]), pitch = u32(env, argv[5]), last = u32(env, argv[6]), S = A.streams(r);
  const int64_t need = samples_needed(layout, S, n, pitch);
  if (need < 0 || (size_t)need > ilen) { napi_throw_range_error(env, nullptr, "input too short"); return nullptr; }
  const size_t n_out = A.by_factor ? (size_t)n * last : last;
  void *out;
  napi_value out_v = make_typed(env, napi_float32_array, n_out * S, 4, &out);
  if (!out_v) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  int rc = A.widen(r, in, format, layout, n, pitch, (float *)out, (A.by_factor || n_out) ? n_out : 1);   // (the library holds a given n_out to its own count)
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return out_v;
}
// (handle, input: Float32Array [S][nIn], nIn, lens: Uint32Array|null, format, layout, factor | nOut) -> the format's typed array, packed
template <class H>
napi_value rate_narrow(napi_env env, napi_callback_info info, const RateApi<H> &A) {
  ARGS(7);
  const int32_t format = i32(env, argv[4]), layout = i32(env, argv[5]);
  if (!sample_format_ok(env, format, layout)) return nullptr;
  H *r = A.of(env, argv[0]);
  if (!r) return nullptr;
  void *in, *lens; size_t ilen, llen;
  if (!typed(env, argv[1], napi_float32_array, &in, &ilen) || !typed(env, argv[3], napi_uint32_array, &lens, &llen, true)) return nullptr;
  const uint32_t n = u32(env, argv[2]), last = u32(env, argv[6]), S = A.streams(r);
  if ((A.by_factor && last == 0) || (size_t)n * S > ilen || (lens && llen < S)) { napi_throw_range_error(env, nullptr, "arguments too short"); return nullptr; }
  const size_t n_out = A.by_factor ? n / last : last, pitch = layout == FSKHIP_LAYOUT_SAMPLE_MAJOR ? S : n_out;
  void *out;
  napi_value out_v = make_typed(env, sample_array_type(format), n_out * S, fskhip_sample_bytes(format), &out);
  if (!out_v) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  int rc = A.narrow(r, (const float *)in, n, n, (const uint32_t *)lens, out, format, layout, pitch ? pitch : 1);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return out_v;
}
template <class H>
napi_value rate_reset(napi_env env, napi_callback_info info, const RateApi<H> &A) {
  ARGS(2);
  H *r = A.of(env, argv[0]);
  if (!r) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = A.reset(r, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
template <class H>
napi_value rate_state(napi_env env, napi_callback_info info, const RateApi<H> &A) {   // -> Float32Array [S][history]
  ARGS(1);
  H *r = A.of(env, argv[0]);
  if (!r) return nullptr;
  void *out;
  napi_value out_v = make_typed(env, napi_float32_array, (size_t)A.streams(r) * A.history(r), 4, &out);
  int rc = A.state_get(r, (float *)out);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return out_v;
}
template <class H>
napi_value rate_set_state(napi_env env, napi_callback_info info, const RateApi<H> &A) {
  ARGS(2);
  H *r = A.of(env, argv[0]);
  if (!r) return nullptr;
  void *st; size_t n;
  if (!typed(env, argv[1], napi_float32_array, &st, &n)) return nullptr;
  if (n != (size_t)A.streams(r) * A.history(r)) { napi_throw_range_error(env, nullptr, "state must be [nStreams][history]"); return nullptr; }
  int rc = A.state_set(r, (const float *)st);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
fskhip_resampler *resampler_of(napi_env env, napi_value v) { return (fskhip_resampler *)filter_of(env, v); }
const RateApi<fskhip_resampler> kResampler = {resampler_of, fskhip_resampler_streams, fskhip_resampler_history, fskhip_resampler_reset, fskhip_resampler_state_get,
                                              fskhip_resampler_state_set, fskhip_resampler_up_host, fskhip_resampler_down_host, true};
napi_value ResamplerHistory(napi_env env, napi_callback_info info) { return rate_count(env, info, kResampler, kResampler.history); }
napi_value ResamplerStreams(napi_env env, napi_callback_info info) { return rate_count(env, info, kResampler, kResampler.streams); }
napi_value ResamplerUp(napi_env env, napi_callback_info info) { return rate_widen(env, info, kResampler); }
napi_value ResamplerDown(napi_env env, napi_callback_info info) { return rate_narrow(env, info, kResampler); }
napi_value ResamplerReset(napi_env env, napi_callback_info info) { return rate_reset(env, info, kResampler); }
napi_value ResamplerState(napi_env env, napi_callback_info info) { return rate_state(env, info, kResampler); }
napi_value ResamplerSetState(napi_env env, napi_callback_info info) { return rate_set_state(env, info, kResampler); }
// process() with both sides at an outer rate: ProcessorProcessSamples with the two handles in front of the samples; lengths and pitches
// count outer rate elements.  Resampler handles go to fskhip_processor_process_rate_host, rate converter handles to
// fskhip_processor_process_ratecvt_host; one call takes one kind.  A handle is looked at only where its side has samples.
FilterBox *rate_box_of(napi_env env, napi_value v) {
  FilterBox *b = (FilterBox *)external(env, v, "filter destroyed");
  if (!b) return nullptr;
  if (!b->p) { napi_throw_error(env, nullptr, "filter destroyed"); return nullptr; }
  if (b->kind != BOX_RESAMPLER && b->kind != BOX_RATECVT) { napi_throw_type_error(env, nullptr, "not a resampler or rate converter handle"); return nullptr; }
  return b;
}
// any_length: fskhip_processor_process_ratecvt_any_host, for rate converters alone
napi_value processor_process_samples_at(napi_env env, napi_callback_info info, bool any_length) {
  ARGS_UPTO(14);
  if (argc < 13) { napi_throw_type_error(env, nullptr, "too few arguments"); return nullptr; }
  const int32_t in_format = i32(env, argv[4]), in_layout = i32(env, argv[5]), out_format = i32(env, argv[8]), out_layout = i32(env, argv[9]);
  if (!sample_format_ok(env, in_format, in_layout) || !sample_format_ok(env, out_format, out_layout)) return nullptr;
  Proc *h = get_proc(env, argv[0]);
  if (!h) return nullptr;
  void *in; size_t ilen;
  if (!typed(env, argv[3], sample_array_type(in_format), &in, &ilen, true)) return nullptr;
  const uint32_t n_in = u32(env, argv[6]), in_pitch = u32(env, argv[7]), n_out = u32(env, argv[10]), out_pitch = u32(env, argv[11]), flags = u32(env, argv[12]);
  FilterBox *up = nullptr, *down = nullptr;
  if (in) {
    if (nullish(env, argv[1])) { napi_throw_type_error(env, nullptr, "input samples need an upsampler"); return nullptr; }
    if (!(up = rate_box_of(env, argv[1]))) return nullptr;
    if (any_length && up->kind != BOX_RATECVT) { napi_throw_type_error(env, nullptr, "quanta of any length take rate converters"); return nullptr; }
    const int64_t need = samples_needed(in_layout, h->S, n_in, in_pitch);
    if (need < 0 || (size_t)need > ilen) { napi_throw_range_error(env, nullptr, "input too short"); return nullptr; }
  }
  void *out = nullptr;
  napi_value out_v = nullptr;
  if (n_out) {
    if (nullish(env, argv[2])) { napi_throw_type_error(env, nullptr, "output samples need a downsampler"); return nullptr; }
    if (!(down = rate_box_of(env, argv[2]))) return nullptr;
    if (any_length && down->kind != BOX_RATECVT) { napi_throw_type_error(env, nullptr, "quanta of any length take rate converters"); return nullptr; }
    if (up && up->kind != down->kind) { napi_throw_type_error(env, nullptr, "one call takes resamplers or rate converters, not one of each"); return nullptr; }
    const int64_t need = samples_needed(out_layout, h->S, n_out, out_pitch);
    if (need < 0) { napi_throw_range_error(env, nullptr, "output pitch too small"); return nullptr; }
    bool fresh = true;
    if (!(out_v = output_array(env, argc > 13, argv[13], sample_array_type(out_format), (size_t)need, fskhip_sample_bytes(out_format), &out, &fresh))) return nullptr;
    if (fresh) fill_silence(out_format, out, (size_t)need);
  }
  void *const uh = up ? up->p : nullptr, *const dh = down ? down->p : nullptr;
  const bool cvt = (up ? up : down) && (up ? up : down)->kind == BOX_RATECVT;
  int rc = any_length ? fskhip_processor_process_ratecvt_any_host(h->p, (fskhip_ratecvt *)uh, (fskhip_ratecvt *)dh, in, in_format, in_layout, n_in, in_pitch, out,
                                                                  out_format, out_layout, n_out, out_pitch, flags)
           : cvt ? fskhip_processor_process_ratecvt_host(h->p, (fskhip_ratecvt *)uh, (fskhip_ratecvt *)dh, in, in_format, in_layout, n_in, in_pitch, out, out_format,
                                                       out_layout, n_out, out_pitch, flags)
               : fskhip_processor_process_rate_host(h->p, (fskhip_resampler *)uh, (fskhip_resampler *)dh, in, in_format, in_layout, n_in, in_pitch, out, out_format,
                                                    out_layout, n_out, out_pitch, flags);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  if (!out_v) napi_get_null(env, &out_v);
  return out_v;
}
napi_value ProcessorProcessSamplesAt(napi_env env, napi_callback_info info) { return processor_process_samples_at(env, info, false); }
napi_value ProcessorProcessSamplesAtAny(napi_env env, napi_callback_info info) { return processor_process_samples_at(env, info, true); }
// ---- rate conversion by a ratio (include/fskhip_next.h: fskhip_ratecvt_*) ----
fskhip_ratecvt *ratecvt_of(napi_env env, napi_value v) {
  FilterBox *b = (FilterBox *)external(env, v, "filter destroyed");
  if (!b) return nullptr;
  if (!b->p) { napi_throw_error(env, nullptr, "filter destroyed"); return nullptr; }
  if (b->kind != BOX_RATECVT) { napi_throw_type_error(env, nullptr, "not a rate converter handle"); return nullptr; }
  return (fskhip_ratecvt *)b->p;
}
napi_value RatecvtCreate(napi_env env, napi_callback_info info) {   // (direction, up, down, taps: Float64Array, nStreams, device, precision)
  ARGS(7);
  void *taps; size_t nt;
  if (!typed(env, argv[3], napi_float64_array, &taps, &nt)) return nullptr;
  fskhip_ratecvt *r = nullptr;
  int rc = fskhip_ratecvt_create(i32(env, argv[5]), i32(env, argv[0]), u32(env, argv[1]), u32(env, argv[2]), (const double *)taps, (uint32_t)nt,
                                 u32(env, argv[4]), i32(env, argv[6]), &r);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return filter_box_new(env, r, BOX_RATECVT);
}
napi_value RatecvtDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  filter_box_close(env, argv[0]);
  return nullptr;
}
const RateApi<fskhip_ratecvt> kRatecvt = {ratecvt_of, fskhip_ratecvt_streams, fskhip_ratecvt_history, fskhip_ratecvt_reset, fskhip_ratecvt_state_get,
                                          fskhip_ratecvt_state_set, fskhip_ratecvt_capture_host, fskhip_ratecvt_playback_host, false};
napi_value RatecvtHistory(napi_env env, napi_callback_info info) { return rate_count(env, info, kRatecvt, kRatecvt.history); }
napi_value RatecvtStreams(napi_env env, napi_callback_info info) { return rate_count(env, info, kRatecvt, kRatecvt.streams); }
napi_value RatecvtCapture(napi_env env, napi_callback_info info) { return rate_widen(env, info, kRatecvt); }
napi_value RatecvtPlayback(napi_env env, napi_callback_info info) { return rate_narrow(env, info, kRatecvt); }
napi_value RatecvtReset(napi_env env, napi_callback_info info) { return rate_reset(env, info, kRatecvt); }
napi_value RatecvtState(napi_env env, napi_callback_info info) { return rate_state(env, info, kRatecvt); }
napi_value RatecvtSetState(napi_env env, napi_callback_info info) { return rate_set_state(env, info, kRatecvt); }
// calls of any length (fskhip_ratecvt_*_any_host): the same marshalling, the output count being the handle's own from its position;
// a call that writes nothing still needs a buffer to name
float g_no_output[4];
int ratecvt_capture_any(fskhip_ratecvt *r, const void *src, int format, int layout, size_t n_in, size_t src_pitch, float *dst, size_t dst_pitch) {
  return fskhip_ratecvt_capture_any_host(r, src, format, layout, n_in, src_pitch, dst ? dst : g_no_output, dst_pitch, nullptr);
}
int ratecvt_playback_any(fskhip_ratecvt *r, const float *src, size_t n_in, size_t src_pitch, const uint32_t *lens, void *dst, int format, int layout, size_t dst_pitch) {
  return fskhip_ratecvt_playback_any_host(r, src, n_in, src_pitch, lens, dst ? dst : (void *)g_no_output, format, layout, dst_pitch, nullptr);
}
const RateApi<fskhip_ratecvt> kRatecvtAny = {ratecvt_of, fskhip_ratecvt_streams, fskhip_ratecvt_history, fskhip_ratecvt_reset, fskhip_ratecvt_state_get,
                                             fskhip_ratecvt_state_set, ratecvt_capture_any, ratecvt_playback_any, false};
napi_value RatecvtCaptureAny(napi_env env, napi_callback_info info) { return rate_widen(env, info, kRatecvtAny); }
napi_value RatecvtPlaybackAny(napi_env env, napi_callback_info info) { return rate_narrow(env, info, kRatecvtAny); }
napi_value RatecvtPosition(napi_env env, napi_callback_info info) { return rate_count(env, info, kRatecvt, fskhip_ratecvt_position); }
napi_value RatecvtSetPosition(napi_env env, napi_callback_info info) {   // (handle, pos)
  ARGS(2);
  fskhip_ratecvt *r = ratecvt_of(env, argv[0]);
  if (!r) return nullptr;
  int rc = fskhip_ratecvt_position_set(r, u32(env, argv[1]));
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
napi_value ratecvt_count_any(napi_env env, napi_callback_info info, size_t (*count)(const fskhip_ratecvt *, size_t)) {   // (handle, n) -> number
  ARGS(2);
  fskhip_ratecvt *r = ratecvt_of(env, argv[0]);
  if (!r) return nullptr;
  napi_value v;
  NAPI_OK(napi_create_double(env, (double)count(r, u32(env, argv[1])), &v));
  return v;
}
napi_value RatecvtOutCountAny(napi_env env, napi_callback_info info) { return ratecvt_count_any(env, info, fskhip_ratecvt_out_count_any); }
napi_value RatecvtInCountAny(napi_env env, napi_callback_info info) { return ratecvt_count_any(env, info, fskhip_ratecvt_in_count_any); }
// ---- a resampler through remap / snapshot / restore (fskhip_resampler_remap ...): remap and restore return a NEW handle
napi_value ResamplerRemap(napi_env env, napi_callback_info info) {   // (handle, map: number[]) -> handle
  ARGS(2);
  fskhip_resampler *r = (fskhip_resampler *)filter_of(env, argv[0]);
  if (!r) return nullptr;
  std::vector<int64_t> map;
  if (!index_array(env, argv[1], "resamplerRemap: map must be an Array of integer stream indices (-1: a new stream)", &map)) return nullptr;
  fskhip_resampler *out = nullptr;
  int rc = fskhip_resampler_remap(r, index_data(map), (uint32_t)map.size(), &out);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return filter_box_new(env, out, BOX_RESAMPLER);
}
napi_value ResamplerSnapshot(napi_env env, napi_callback_info info) {   // (handle, streams: number[]|null) -> Buffer
  ARGS(2);
  fskhip_resampler *r = (fskhip_resampler *)filter_of(env, argv[0]);
  if (!r) return nullptr;
  std::vector<int64_t> sel;
  const bool all = nullish(env, argv[1]);
  if (!all && !index_array(env, argv[1], "resamplerSnapshot: streams must be an Array of integer stream indices", &sel)) return nullptr;
  const uint32_t n = all ? fskhip_resampler_streams(r) : (uint32_t)sel.size();
  size_t need = 0;
  int rc = fskhip_resampler_snapshot_bytes(r, n, &need);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  void *data = nullptr;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, need, &data, &buf));
  rc = fskhip_resampler_snapshot(r, index_data(sel, all), n, data, need, nullptr);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return buf;
}
napi_value ResamplerRestore(napi_env env, napi_callback_info info) {   // (snapshot: Uint8Array, map: number[]|null, device) -> handle
  ARGS(3);
  void *data; size_t size;
  if (!typed(env, argv[0], napi_uint8_array, &data, &size)) return nullptr;
  std::vector<int64_t> map;
  const bool all = nullish(env, argv[1]);
  if (!all && !index_array(env, argv[1], "resamplerRestore: map must be an Array of integer record indices (-1: a new stream)", &map)) return nullptr;
  fskhip_resampler *out = nullptr;
  int rc = fskhip_resampler_restore(i32(env, argv[2]), data, size, index_data(map, all), (uint32_t)map.size(), &out);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return filter_box_new(env, out, BOX_RESAMPLER);
}
napi_value ResamplerSnapshotInfo(napi_env env, napi_callback_info info) {   // (snapshot) -> {nStreams, direction, factor, nTaps, precision, history, taps}
  ARGS(1);
  void *data; size_t size;
  if (!typed(env, argv[0], napi_uint8_array, &data, &size)) return nullptr;
  fskhip_resampler_snapshot_info si;
  int rc = fskhip_resampler_snapshot_info_get(data, size, &si);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  set_u32(env, o, "nStreams", si.n_streams);
  set_u32(env, o, "direction", (uint32_t)si.direction);
  set_u32(env, o, "factor", si.factor);
  set_u32(env, o, "nTaps", si.n_taps);
  set_u32(env, o, "precision", (uint32_t)si.precision);
  set_u32(env, o, "history", si.history);
  void *taps;   // (behind the 48-byte header of a validated image)
  napi_value taps_v = make_typed(env, napi_float64_array, si.n_taps, 8, &taps);
  memcpy(taps, (const unsigned char *)data + 48, sizeof(double) * (size_t)si.n_taps);
  napi_set_named_property(env, o, "taps", taps_v);
  return o;
}
// ---- a rate converter through remap / snapshot / restore (fskhip_ratecvt_remap ...): the resampler's four, over its own C calls
napi_value RatecvtRemap(napi_env env, napi_callback_info info) {   // (handle, map: number[]) -> handle
  ARGS(2);
  fskhip_ratecvt *r = ratecvt_of(env, argv[0]);
  if (!r) return nullptr;
  std::vector<int64_t> map;
  if (!index_array(env, argv[1], "ratecvtRemap: map must be an Array of integer stream indices (-1: a new stream)", &map)) return nullptr;
  fskhip_ratecvt *out = nullptr;
  int rc = fskhip_ratecvt_remap(r, index_data(map), (uint32_t)map.size(), &out);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return filter_box_new(env, out, BOX_RATECVT);
}
napi_value RatecvtSnapshot(napi_env env, napi_callback_info info) {   // (handle, streams: number[]|null) -> Buffer
  ARGS(2);
  fskhip_ratecvt *r = ratecvt_of(env, argv[0]);
  if (!r) return nullptr;
  std::vector<int64_t> sel;
  const bool all = nullish(env, argv[1]);
  if (!all && !index_array(env, argv[1], "ratecvtSnapshot: streams must be an Array of integer stream indices", &sel)) return nullptr;
  const uint32_t n = all ? fskhip_ratecvt_streams(r) : (uint32_t)sel.size();
  size_t need = 0;
  int rc = fskhip_ratecvt_snapshot_bytes(r, n, &need);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  void *data = nullptr;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, need, &data, &buf));
  rc = fskhip_ratecvt_snapshot(r, index_data(sel, all), n, data, need, nullptr);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return buf;
}
napi_value RatecvtRestore(napi_env env, napi_callback_info info) {   // (snapshot: Uint8Array, map: number[]|null, device) -> handle
  ARGS(3);
  void *data; size_t size;
  if (!typed(env, argv[0], napi_uint8_array, &data, &size)) return nullptr;
  std::vector<int64_t> map;
  const bool all = nullish(env, argv[1]);
  if (!all && !index_array(env, argv[1], "ratecvtRestore: map must be an Array of integer record indices (-1: a new stream)", &map)) return nullptr;
  fskhip_ratecvt *out = nullptr;
  int rc = fskhip_ratecvt_restore(i32(env, argv[2]), data, size, index_data(map, all), (uint32_t)map.size(), &out);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return filter_box_new(env, out, BOX_RATECVT);
}
napi_value RatecvtSnapshotInfo(napi_env env, napi_callback_info info) {   // (snapshot) -> {nStreams, direction, up, down, nTaps, precision, history, position, taps}
  ARGS(1);
  void *data; size_t size;
  if (!typed(env, argv[0], napi_uint8_array, &data, &size)) return nullptr;
  fskhip_ratecvt_snapshot_info si;
  int rc = fskhip_ratecvt_snapshot_info_get(data, size, &si);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  set_u32(env, o, "nStreams", si.n_streams);
  set_u32(env, o, "direction", (uint32_t)si.direction);
  set_u32(env, o, "up", si.up);
  set_u32(env, o, "down", si.down);
  set_u32(env, o, "nTaps", si.n_taps);
  set_u32(env, o, "precision", (uint32_t)si.precision);
  set_u32(env, o, "history", si.history);
  set_u32(env, o, "position", si.position);
  void *taps;   // (behind the 64-byte header of a validated image)
  napi_value taps_v = make_typed(env, napi_float64_array, si.n_taps, 8, &taps);
  memcpy(taps, (const unsigned char *)data + 64, sizeof(double) * (size_t)si.n_taps);
  napi_set_named_property(env, o, "taps", taps_v);
  return o;
}

// ---- IIRFilter (src/dsp/filters.ts:8-106) ----
napi_value IirCreate(napi_env env, napi_callback_info info) {   // (b: Float64Array, a: Float64Array, nStreams, device, precision)
  ARGS(5);
  void *b, *a; size_t nb, na;
  if (!typed(env, argv[0], napi_float64_array, &b, &nb) || !typed(env, argv[1], napi_float64_array, &a, &na)) return nullptr;
  fskhip_iir *f = nullptr;
  int rc = fskhip_iir_create(i32(env, argv[3]), (const double *)b, (uint32_t)nb, (const double *)a, (uint32_t)na, u32(env, argv[2]), i32(env, argv[4]), &f);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return filter_box_new(env, f, BOX_IIR);
}
napi_value IirDestroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  filter_box_close(env, argv[0]);
  return nullptr;
}
napi_value IirCoefficients(napi_env env, napi_callback_info info) {   // -> Float64Array [nb, na, b..., a...]
  ARGS(1);
  fskhip_iir *f = (fskhip_iir *)filter_of(env, argv[0]);
  if (!f) return nullptr;
  double b[9], a[9];
  uint32_t nb = 0, na = 0;
  int rc = fskhip_iir_get_coefficients(f, b, &nb, a, &na);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  void *out;
  napi_value out_v = make_typed(env, napi_float64_array, 2 + nb + na, 8, &out);
  double *o = (double *)out;
  o[0] = nb; o[1] = na;
  for (uint32_t i = 0; i < nb; i++) o[2 + i] = b[i];
  for (uint32_t i = 0; i < na; i++) o[2 + nb + i] = a[i];
  return out_v;
}
napi_value IirProcess(napi_env env, napi_callback_info info) {   // Float32Array in -> Float32Array (processBuffer); Float64Array in -> Float64Array (process)
  ARGS(5);
  fskhip_iir *f = (fskhip_iir *)filter_of(env, argv[0]);
  if (!f) return nullptr;
  napi_typedarray_type ty; size_t ilen; void *in; napi_value ab; size_t off;
  if (napi_get_typedarray_info(env, argv[1], &ty, &ilen, &in, &ab, &off) != napi_ok || (ty != napi_float32_array && ty != napi_float64_array)) {
    napi_throw_type_error(env, nullptr, "Float32Array or Float64Array expected");
    return nullptr;
  }
  const uint32_t n = u32(env, argv[2]), pitch = u32(env, argv[3]), S = u32(env, argv[4]);
  if (S != fskhip_iir_streams(f)) { napi_throw_range_error(env, nullptr, "nStreams is not the filter's stream count"); return nullptr; }
  if (S == 0 || pitch < n || (size_t)pitch * (S - 1) + n > ilen) { napi_throw_range_error(env, nullptr, "input too short"); return nullptr; }
  void *out;
  int rc;
  napi_value out_v;
  if (ty == napi_float32_array) {
    out_v = make_typed(env, napi_float32_array, (size_t)n * S, 4, &out);
    rc = fskhip_iir_process_host(f, (const float *)in, n, pitch, (float *)out, n);
  } else {
    out_v = make_typed(env, napi_float64_array, (size_t)n * S, 8, &out);
    rc = fskhip_iir_process_f64_host(f, (const double *)in, n, pitch, (double *)out, n);
  }
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return out_v;
}
napi_value IirReset(napi_env env, napi_callback_info info) {
  ARGS(2);
  fskhip_iir *f = (fskhip_iir *)filter_of(env, argv[0]);
  if (!f) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = fskhip_iir_reset(f, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
napi_value Butterworth(napi_env env, napi_callback_info info) {   // (kind 0 lowpass | 1 highpass | 2 bandpass, f, [bandwidth,] sampleRate) -> Float64Array [b0 b1 b2 a0 a1 a2]
  ARGS(4);
  const int kind = i32(env, argv[0]);
  double b[3], a[3];
  if (kind == 0) fskhip_butterworth_lowpass(f64(env, argv[1]), f64(env, argv[3]), b, a);
  else if (kind == 1) fskhip_butterworth_highpass(f64(env, argv[1]), f64(env, argv[3]), b, a);
  else fskhip_butterworth_bandpass(f64(env, argv[1]), f64(env, argv[2]), f64(env, argv[3]), b, a);
  void *out;
  napi_value out_v = make_typed(env, napi_float64_array, 6, 8, &out);
  double *o = (double *)out;
  for (int i = 0; i < 3; i++) { o[i] = b[i]; o[3 + i] = a[i]; }
  return out_v;
}

}  // namespace

napi_value InitNext(napi_env env, napi_value exports) {
  const napi_property_descriptor props[] = {
      {"crc16", nullptr, Crc16, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemSerialize", nullptr, XmodemSerialize, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemScan", nullptr, XmodemScan, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorCreate", nullptr, ProcessorCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorDestroy", nullptr, ProcessorDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorProcess", nullptr, ProcessorProcess, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorProcessSamples", nullptr, ProcessorProcessSamples, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorModulate", nullptr, ProcessorModulate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorTxState", nullptr, ProcessorTxState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorRxLength", nullptr, ProcessorRxLength, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorLastTxKernel", nullptr, ProcessorLastTxKernel, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorDrain", nullptr, ProcessorDrain, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorDrainSparse", nullptr, ProcessorDrainSparse, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorReset", nullptr, ProcessorReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxCreate", nullptr, XmodemRxCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxDestroy", nullptr, XmodemRxDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxPoll", nullptr, XmodemRxPoll, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxReset", nullptr, XmodemRxReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxState", nullptr, XmodemRxState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxSetState", nullptr, XmodemRxSetState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxCreate", nullptr, XmodemTxCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxDestroy", nullptr, XmodemTxDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxSend", nullptr, XmodemTxSend, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxPoll", nullptr, XmodemTxPoll, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxReset", nullptr, XmodemTxReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxState", nullptr, XmodemTxState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxSetState", nullptr, XmodemTxSetState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvCreate", nullptr, XmodemRecvCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvDestroy", nullptr, XmodemRecvDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvStart", nullptr, XmodemRecvStart, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvPoll", nullptr, XmodemRecvPoll, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvReset", nullptr, XmodemRecvReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvFiles", nullptr, XmodemRecvFiles, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvSetFiles", nullptr, XmodemRecvSetFiles, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvState", nullptr, XmodemRecvState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvSetState", nullptr, XmodemRecvSetState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerCreate", nullptr, XmodemTimerCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerDestroy", nullptr, XmodemTimerDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerPoll", nullptr, XmodemTimerPoll, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerReset", nullptr, XmodemTimerReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerState", nullptr, XmodemTimerState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerSetState", nullptr, XmodemTimerSetState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorRemap", nullptr, ProcessorRemap, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorSnapshot", nullptr, ProcessorSnapshot, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorRestore", nullptr, ProcessorRestore, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorSnapshotInfo", nullptr, ProcessorSnapshotInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorSnapshotConcat", nullptr, ProcessorSnapshotConcat, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxRemap", nullptr, XmodemRxRemap, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxSnapshot", nullptr, XmodemRxSnapshot, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRxRestore", nullptr, XmodemRxRestore, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxRemap", nullptr, XmodemTxRemap, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxSnapshot", nullptr, XmodemTxSnapshot, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTxRestore", nullptr, XmodemTxRestore, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvRemap", nullptr, XmodemRecvRemap, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvSnapshot", nullptr, XmodemRecvSnapshot, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemRecvRestore", nullptr, XmodemRecvRestore, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemSnapshotInfo", nullptr, XmodemSnapshotInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerRemap", nullptr, XmodemTimerRemap, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerSnapshot", nullptr, XmodemTimerSnapshot, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerRestore", nullptr, XmodemTimerRestore, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"xmodemTimerSnapshotInfo", nullptr, XmodemTimerSnapshotInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"sincLowpass", nullptr, SincLowpass, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"sincHighpass", nullptr, SincHighpass, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"sincBandpass", nullptr, SincBandpass, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"firCreate", nullptr, FirCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"firDestroy", nullptr, FirDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"firProcess", nullptr, FirProcess, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"firReset", nullptr, FirReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerCreate", nullptr, ResamplerCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerDestroy", nullptr, ResamplerDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerHistory", nullptr, ResamplerHistory, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerUp", nullptr, ResamplerUp, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerDown", nullptr, ResamplerDown, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorProcessSamplesAt", nullptr, ProcessorProcessSamplesAt, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerReset", nullptr, ResamplerReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerState", nullptr, ResamplerState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerSetState", nullptr, ResamplerSetState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerStreams", nullptr, ResamplerStreams, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerRemap", nullptr, ResamplerRemap, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerSnapshot", nullptr, ResamplerSnapshot, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerRestore", nullptr, ResamplerRestore, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"resamplerSnapshotInfo", nullptr, ResamplerSnapshotInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtCreate", nullptr, RatecvtCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtDestroy", nullptr, RatecvtDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtHistory", nullptr, RatecvtHistory, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtStreams", nullptr, RatecvtStreams, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtCapture", nullptr, RatecvtCapture, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtPlayback", nullptr, RatecvtPlayback, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtReset", nullptr, RatecvtReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtState", nullptr, RatecvtState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtSetState", nullptr, RatecvtSetState, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtCaptureAny", nullptr, RatecvtCaptureAny, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtPlaybackAny", nullptr, RatecvtPlaybackAny, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtPosition", nullptr, RatecvtPosition, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtSetPosition", nullptr, RatecvtSetPosition, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtOutCountAny", nullptr, RatecvtOutCountAny, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtInCountAny", nullptr, RatecvtInCountAny, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtRemap", nullptr, RatecvtRemap, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtSnapshot", nullptr, RatecvtSnapshot, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtRestore", nullptr, RatecvtRestore, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ratecvtSnapshotInfo", nullptr, RatecvtSnapshotInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"processorProcessSamplesAtAny", nullptr, ProcessorProcessSamplesAtAny, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"iirCreate", nullptr, IirCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"iirDestroy", nullptr, IirDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"iirCoefficients", nullptr, IirCoefficients, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"iirProcess", nullptr, IirProcess, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"iirReset", nullptr, IirReset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"butterworth", nullptr, Butterworth, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}
