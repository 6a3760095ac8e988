// fsk_addon.cc -- thin N-API binding of the C ABI in include/fskhip.h.
//
// This is the FFI a reference maintainer would add: FSKCore / FSKProcessor keep their
// TypeScript signatures and call these functions; nothing here computes DSP.  Built directly against
// /usr/include/node/node_api.h with g++ (no node-gyp download), linked to libfskhip.so.
// What an entry point is spelled with -- ARGS_UPTO, u32 / i32, make_typed, index_array, set_num, throw_fsk -- is addon_util.h's,
// shared with fsk_addon_next.cc; this file adds the FSKConfig conversion, the busy-engine bookkeeping and get_blob.
//
// JS surface (all synchronous; errors throw with the C library's message):
//   create(configs: object | object[], nStreams, device, precision) -> handle
//   destroy(handle)
//   demodulate(handle, samples: Float32Array, nPerStream, pitch, flags) -> {out: Uint8Array, outPitch, counts: Uint32Array, eod: Uint32Array}
//   demodulateAsync(... same ...) -> Promise of the same object; runs on a libuv worker thread
//   demodulateSamples(handle, samples: Int16Array | Uint8Array | Float32Array, format, layout, nPerStream, pitch) -> the same object:
//     capture samples as they arrive (FSKHIP_SAMPLES_* / FSKHIP_LAYOUT_*, fskhip_demodulate_host_fmt); demodulateSamplesAsync likewise
//   modulateSamples(handle, payloads, lens, payloadPitch, format, layout, nPerStream, pitch, out | null) -> {out, lens}: the same formats
//     out (fskhip_modulate_host_fmt)
//   modulate(handle, payloads: Uint8Array, lens: Uint32Array, payloadPitch) -> {out: Float32Array, outPitch, lens: Uint32Array}
//   modulatedLength(handle, nBytes) -> number
//   reset(handle, stream)            stream < 0: all
//   getStatus(handle, stream) -> {ready, frameStarted, globalSampleCounter, ...}
//   demodSupported(handle) -> boolean
//   deviceCount() -> number
#include <cstring>
#include <string>
#include <vector>

#include "addon_util.h"

static bool get_number(napi_env env, napi_value obj, const char *key, double *out) {
  bool has = false;
  if (napi_has_named_property(env, obj, key, &has) != napi_ok || !has) return false;
  napi_value v;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok) return false;
  napi_valuetype t;
  napi_typeof(env, v, &t);
  if (t == napi_boolean) { bool b; napi_get_value_bool(env, v, &b); *out = b ? 1 : 0; return true; }
  if (t != napi_number) return false;
  return napi_get_value_double(env, v, out) == napi_ok;
}

static bool get_bytes(napi_env env, napi_value obj, const char *key, int32_t *dst, int32_t *len) {
  bool has = false;
  if (napi_has_named_property(env, obj, key, &has) != napi_ok || !has) return true;
  napi_value arr;
  napi_get_named_property(env, obj, key, &arr);
  bool is_arr = false;
  napi_is_array(env, arr, &is_arr);
  if (!is_arr) return false;
  uint32_t n = 0;
  napi_get_array_length(env, arr, &n);
  if (n > FSKHIP_MAX_PATTERN_BYTES) return false;
  for (uint32_t i = 0; i < n; i++) {
    napi_value e;
    napi_get_element(env, arr, i, &e);
    double d = 0;
    napi_get_value_double(env, e, &d);
    dst[i] = (int32_t)d;
  }
  *len = (int32_t)n;
  return true;
}

// FSKConfig object (reference field names, partial objects merge over DEFAULT_FSK_CONFIG like
// configure() does, fsk.ts:134) -> fskhip_config
static bool to_config(napi_env env, napi_value obj, fskhip_config *c) {
  fskhip_default_config(c);
  double d;
  if (get_number(env, obj, "sampleRate", &d)) c->sampleRate = d;
  if (get_number(env, obj, "baudRate", &d)) c->baudRate = d;
  if (get_number(env, obj, "markFrequency", &d)) c->markFrequency = d;
  if (get_number(env, obj, "spaceFrequency", &d)) c->spaceFrequency = d;
  if (get_number(env, obj, "startBits", &d)) c->startBits = (int32_t)d;
  if (get_number(env, obj, "stopBits", &d)) c->stopBits = (int32_t)d;
  if (get_number(env, obj, "syncThreshold", &d)) c->syncThreshold = d;
  if (get_number(env, obj, "agcEnabled", &d)) c->agcEnabled = d != 0;
  if (get_number(env, obj, "preFilterBandwidth", &d)) c->preFilterBandwidth = d;
  if (get_number(env, obj, "adaptiveThreshold", &d)) c->adaptiveThreshold = d != 0;
  if (!get_bytes(env, obj, "preamblePattern", c->preamblePattern, &c->preambleLen)) return false;
  if (!get_bytes(env, obj, "sfdPattern", c->sfdPattern, &c->sfdLen)) return false;
  bool has = false;
  napi_has_named_property(env, obj, "parity", &has);
  if (has) {
    napi_value v;
    napi_get_named_property(env, obj, "parity", &v);
    char buf[16] = {0};
    size_t n = 0;
    if (napi_get_value_string_utf8(env, v, buf, sizeof(buf), &n) == napi_ok) {
      c->parity = !strcmp(buf, "even") ? 1 : !strcmp(buf, "odd") ? 2 : 0;
    }
  }
  return true;
}

// Engines with a demodulateAsync call in flight on a libuv worker (touched on the JS thread only).  EVERY entry point
// that takes the engine handle goes through get_engine(), which refuses a busy engine: the worker is inside
// fskhip_demodulate_host with the engine's staging buffers and host-side counters.  destroy() of a busy engine is
// deferred until its call completes.
static std::vector<fskhip_engine *> g_busy;
static std::vector<fskhip_engine *> g_doomed;
static bool is_busy(const fskhip_engine *e) {
  for (const fskhip_engine *b : g_busy)
    if (b == e) return true;
  return false;
}
static fskhip_engine *get_engine(napi_env env, napi_value v) {
  fskhip_engine *e = (fskhip_engine *)external(env, v, "FSK modulator not configured");
  if (e && is_busy(e)) {
    napi_throw_error(env, nullptr, "an asynchronous call is already in flight on this engine");
    return nullptr;
  }
  return e;
}

static napi_value Create(napi_env env, napi_callback_info info) {
  ARGS_UPTO(4);
  if (argc < 4) { napi_throw_type_error(env, nullptr, "create(configs, nStreams, device, precision)"); return nullptr; }
  const uint32_t n_streams = u32(env, argv[1]);
  const int32_t device = i32(env, argv[2]), precision = i32(env, argv[3]);
  std::vector<fskhip_config> cfgs;
  bool is_arr = false;
  napi_is_array(env, argv[0], &is_arr);
  if (is_arr) {
    uint32_t n = 0;
    napi_get_array_length(env, argv[0], &n);
    cfgs.resize(n);
    for (uint32_t i = 0; i < n; i++) {
      napi_value e;
      napi_get_element(env, argv[0], i, &e);
      if (!to_config(env, e, &cfgs[i])) { napi_throw_type_error(env, nullptr, "bad FSKConfig"); return nullptr; }
    }
  } else {
    cfgs.resize(1);
    if (!to_config(env, argv[0], &cfgs[0])) { napi_throw_type_error(env, nullptr, "bad FSKConfig"); return nullptr; }
  }
  fskhip_engine *e = nullptr;
  int rc = fskhip_create(cfgs.data(), (uint32_t)cfgs.size(), n_streams, device, precision, &e);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value ext;
  NAPI_OK(napi_create_external(env, e, nullptr, nullptr, &ext));
  return ext;
}

static napi_value Destroy(napi_env env, napi_callback_info info) {
  ARGS_UPTO(1);
  void *p = nullptr;
  if (argc == 1 && napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
    if (is_busy((fskhip_engine *)p)) g_doomed.push_back((fskhip_engine *)p);   // destroyed by demod_complete
    else fskhip_destroy((fskhip_engine *)p);
  }
  return nullptr;
}

// demodulateData (fsk.ts:190-222) for every stream.  The input Float32Array is BORROWED for the call
// (napi_get_typedarray_info, never retained); with flags & 1 it is overwritten with the AGC-scaled
// samples like the reference does (fsk.ts:55).
// What demodulate and demodulateAsync share: one call's arguments, validated, and its outputs, allocated ...
struct DemodCall {
  fskhip_engine *e = nullptr;
  void *samples = nullptr;
  int32_t format = FSKHIP_SAMPLES_F32, layout = FSKHIP_LAYOUT_STREAM_MAJOR;   // (as they are: fskhip_demodulate_host's own call)
  uint8_t *out = nullptr;
  uint32_t *counts = nullptr, *eod = nullptr;
  uint32_t n = 0, pitch = 0, flags = 0;
  size_t out_pitch = 0;
};
struct DemodArrays { napi_value samples, out, counts, eod; };
// fmt: the arguments of demodulateSamples (handle, samples, format, layout, nPerStream, pitch) instead of demodulate's
static DemodCall *demod_prepare(napi_env env, napi_callback_info info, DemodCall *c, DemodArrays *a, bool fmt = false) {   // (nullptr: thrown)
  ARGS_UPTO(6);
  c->e = get_engine(env, argv[0]);
  if (!c->e) return nullptr;
  napi_typedarray_type tt;
  size_t len = 0;
  void *data = nullptr;
  NAPI_OK(napi_get_typedarray_info(env, argv[1], &tt, &len, &data, nullptr, nullptr));
  if (fmt) {
    c->format = i32(env, argv[2]); c->layout = i32(env, argv[3]);
    c->n = u32(env, argv[4]); c->pitch = u32(env, argv[5]);
    if (!sample_format_ok(env, c->format, c->layout)) return nullptr;
    if (tt != sample_array_type(c->format)) { napi_throw_type_error(env, nullptr, "samples must be the format's typed array: Float32Array, Int16Array or (G.711) Uint8Array"); return nullptr; }
  } else {
    if (tt != napi_float32_array) { napi_throw_type_error(env, nullptr, "samples must be a Float32Array"); return nullptr; }
    c->n = u32(env, argv[2]); c->pitch = u32(env, argv[3]); c->flags = u32(env, argv[4]);
  }
  c->samples = data;
  const uint32_t S = fskhip_n_streams(c->e);
  // the last row (stream-major) / the last frame (sample-major) may end with its own samples
  const bool frames = c->layout == FSKHIP_LAYOUT_SAMPLE_MAJOR;
  const size_t rows = frames ? c->n : S, cols = frames ? S : c->n;
  if (c->pitch < cols || (rows && (size_t)c->pitch * (rows - 1) + cols > len)) { napi_throw_range_error(env, nullptr, "samples too short"); return nullptr; }
  c->out_pitch = fskhip_max_bytes(c->e, c->n);  // the library's own bound (a byte needs >= 8 bit times of samplesPerBit samples)
  void *out = nullptr, *counts = nullptr, *eod = nullptr;
  a->samples = argv[1];
  a->out = make_typed(env, napi_uint8_array, c->out_pitch * S, 1, &out);
  a->counts = make_typed(env, napi_uint32_array, S, 4, &counts);
  a->eod = make_typed(env, napi_uint32_array, S, 4, &eod);
  if (!a->out || !a->counts || !a->eod) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  c->out = (uint8_t *)out; c->counts = (uint32_t *)counts; c->eod = (uint32_t *)eod;
  return c;
}
// ... and the object both hand back
static napi_value demod_result(napi_env env, size_t out_pitch, napi_value out_v, napi_value cnt_v, napi_value eod_v) {
  napi_value res;
  NAPI_OK(napi_create_object(env, &res));
  napi_set_named_property(env, res, "out", out_v);
  set_u32(env, res, "outPitch", (uint32_t)out_pitch);
  napi_set_named_property(env, res, "counts", cnt_v);
  napi_set_named_property(env, res, "eod", eod_v);
  return res;
}

// (format F32 in stream-major layout IS fskhip_demodulate_host, write-back flag included: include/fskhip.h)
static int demod_run(const DemodCall &c) {
  return fskhip_demodulate_host_fmt(c.e, c.samples, c.format, c.layout, c.n, c.pitch, c.out, c.out_pitch, c.counts, c.eod, c.flags);
}
static napi_value demodulate_sync(napi_env env, napi_callback_info info, bool fmt) {
  DemodCall c;
  DemodArrays a;
  if (!demod_prepare(env, info, &c, &a, fmt)) return nullptr;
  int rc = demod_run(c);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return demod_result(env, c.out_pitch, a.out, a.counts, a.eod);
}
static napi_value Demodulate(napi_env env, napi_callback_info info) { return demodulate_sync(env, info, false); }
static napi_value DemodulateSamples(napi_env env, napi_callback_info info) { return demodulate_sync(env, info, true); }

// demodulateAsync: the same call on a libuv worker thread, for batches big enough to matter to the event loop
// (SURVEY 8b "Threading").  Output arrays are created up front on the JS thread; the input Float32Array is
// referenced until the work completes.  One call in flight per engine: a second one rejects.
struct DemodWork {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  napi_ref in_ref = nullptr, out_ref = nullptr, cnt_ref = nullptr, eod_ref = nullptr;
  DemodCall c;
  int rc = 0;
  std::string err;
};
static void demod_execute(napi_env, void *data) {
  DemodWork *w = (DemodWork *)data;
  const DemodCall &c = w->c;
  w->rc = demod_run(c);
  if (w->rc != FSKHIP_OK) w->err = fskhip_last_error();  // thread-local: read it on the thread that failed
}
static void demod_complete(napi_env env, napi_status, void *data) {
  DemodWork *w = (DemodWork *)data;
  for (size_t i = 0; i < g_busy.size(); i++)
    if (g_busy[i] == w->c.e) { g_busy.erase(g_busy.begin() + i); break; }
  bool doomed = false;
  for (size_t i = 0; i < g_doomed.size(); i++)
    if (g_doomed[i] == w->c.e) { g_doomed.erase(g_doomed.begin() + i); doomed = true; break; }
  if (w->rc == FSKHIP_OK) {
    napi_value out_v, cnt_v, eod_v;
    napi_get_reference_value(env, w->out_ref, &out_v);
    napi_get_reference_value(env, w->cnt_ref, &cnt_v);
    napi_get_reference_value(env, w->eod_ref, &eod_v);
    napi_resolve_deferred(env, w->deferred, demod_result(env, w->c.out_pitch, out_v, cnt_v, eod_v));
  } else {
    napi_value msg, errv;
    napi_create_string_utf8(env, w->err.c_str(), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, nullptr, msg, &errv);
    napi_reject_deferred(env, w->deferred, errv);
  }
  napi_delete_reference(env, w->in_ref);
  napi_delete_reference(env, w->out_ref);
  napi_delete_reference(env, w->cnt_ref);
  napi_delete_reference(env, w->eod_ref);
  napi_delete_async_work(env, w->work);
  if (doomed) fskhip_destroy(w->c.e);   // destroy() was called while the worker held the engine
  delete w;
}

static napi_value demodulate_async(napi_env env, napi_callback_info info, bool fmt) {
  DemodCall c;
  DemodArrays a;
  if (!demod_prepare(env, info, &c, &a, fmt)) return nullptr;
  DemodWork *w = new DemodWork();
  w->c = c;
  napi_create_reference(env, a.samples, 1, &w->in_ref);
  napi_create_reference(env, a.out, 1, &w->out_ref);
  napi_create_reference(env, a.counts, 1, &w->cnt_ref);
  napi_create_reference(env, a.eod, 1, &w->eod_ref);
  napi_value promise, name;
  napi_create_promise(env, &w->deferred, &promise);
  napi_create_string_utf8(env, "fskhip_demodulate", NAPI_AUTO_LENGTH, &name);
  napi_create_async_work(env, nullptr, name, demod_execute, demod_complete, w, &w->work);
  g_busy.push_back(c.e);
  napi_queue_async_work(env, w->work);
  return promise;
}
static napi_value DemodulateAsync(napi_env env, napi_callback_info info) { return demodulate_async(env, info, false); }
static napi_value DemodulateSamplesAsync(napi_env env, napi_callback_info info) { return demodulate_async(env, info, true); }

// modulateData (fsk.ts:377-424) for every stream
static napi_value Modulate(napi_env env, napi_callback_info info) {
  ARGS_UPTO(4);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  napi_typedarray_type tt;
  size_t plen = 0, llen = 0;
  void *pdata = nullptr, *ldata = nullptr;
  NAPI_OK(napi_get_typedarray_info(env, argv[1], &tt, &plen, &pdata, nullptr, nullptr));
  if (tt != napi_uint8_array) { napi_throw_type_error(env, nullptr, "payloads must be a Uint8Array"); return nullptr; }
  NAPI_OK(napi_get_typedarray_info(env, argv[2], &tt, &llen, &ldata, nullptr, nullptr));
  if (tt != napi_uint32_array) { napi_throw_type_error(env, nullptr, "lens must be a Uint32Array"); return nullptr; }
  const uint32_t ppitch = u32(env, argv[3]);
  const uint32_t S = fskhip_n_streams(e);
  if (llen < S || plen < (size_t)ppitch * S) { napi_throw_range_error(env, nullptr, "payloads/lens too short"); return nullptr; }
  uint32_t max_len = 0;
  for (uint32_t s = 0; s < S; s++) max_len = ((uint32_t *)ldata)[s] > max_len ? ((uint32_t *)ldata)[s] : max_len;
  size_t out_pitch = fskhip_modulated_length(e, max_len);
  if (out_pitch < 4) out_pitch = 4;
  void *out = nullptr, *olens = nullptr;
  napi_value out_v = make_typed(env, napi_float32_array, out_pitch * S, 4, &out);
  napi_value len_v = make_typed(env, napi_uint32_array, S, 4, &olens);
  if (!out_v || !len_v) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  int rc = fskhip_modulate_host(e, (const uint8_t *)pdata, (const uint32_t *)ldata, ppitch, (float *)out, out_pitch,
                                (uint32_t *)olens);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value res;
  NAPI_OK(napi_create_object(env, &res));
  napi_set_named_property(env, res, "out", out_v);
  set_u32(env, res, "outPitch", (uint32_t)out_pitch);
  napi_set_named_property(env, res, "lens", len_v);
  return res;
}

// modulateSamples(handle, payloads: Uint8Array, lens: Uint32Array, payloadPitch, format, layout, nPerStream, pitch, out | null) ->
// {out, lens}: modulateData into playback samples (fskhip_modulate_host_fmt) -- an Int16Array, a G.711 Uint8Array or a Float32Array,
// stream-major [S][pitch] or interleaved frames [nPerStream][pitch >= S].  `out`: the caller's array of that type (a shard passes
// the frames from its first column on), written in place; null: a new one.  Argument checks as demodulateSamples makes them.
static napi_value ModulateSamples(napi_env env, napi_callback_info info) {
  ARGS_UPTO(9);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  napi_typedarray_type tt;
  size_t plen = 0, llen = 0, olen = 0;
  void *pdata = nullptr, *ldata = nullptr, *out = nullptr, *olens = nullptr;
  NAPI_OK(napi_get_typedarray_info(env, argv[1], &tt, &plen, &pdata, nullptr, nullptr));
  if (tt != napi_uint8_array) { napi_throw_type_error(env, nullptr, "payloads must be a Uint8Array"); return nullptr; }
  NAPI_OK(napi_get_typedarray_info(env, argv[2], &tt, &llen, &ldata, nullptr, nullptr));
  if (tt != napi_uint32_array) { napi_throw_type_error(env, nullptr, "lens must be a Uint32Array"); return nullptr; }
  const uint32_t ppitch = u32(env, argv[3]);
  const int32_t format = i32(env, argv[4]), layout = i32(env, argv[5]);
  const uint32_t n = u32(env, argv[6]), pitch = u32(env, argv[7]);
  const uint32_t S = fskhip_n_streams(e);
  if (llen < S || plen < (size_t)ppitch * S) { napi_throw_range_error(env, nullptr, "payloads/lens too short"); return nullptr; }
  if (!sample_format_ok(env, format, layout)) return nullptr;
  const size_t esz = fskhip_sample_bytes(format);
  const napi_typedarray_type want = sample_array_type(format);
  // the last row (stream-major) / the last frame (sample-major) may end with its own samples
  const bool frames = layout == FSKHIP_LAYOUT_SAMPLE_MAJOR;
  const size_t rows = frames ? n : S, cols = frames ? S : n;
  const size_t need = rows ? (size_t)pitch * (rows - 1) + cols : 0;
  napi_value out_v = argv[8];
  if (argc < 9 || nullish(env, argv[8])) {
    if (pitch < cols) { napi_throw_range_error(env, nullptr, "samples too short"); return nullptr; }
    out_v = make_typed(env, want, need, esz, &out);
    if (!out_v) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
    fill_silence(format, out, need);   // (the pitch's padding: silence, like the rest)
  } else {
    NAPI_OK(napi_get_typedarray_info(env, argv[8], &tt, &olen, &out, nullptr, nullptr));
    if (tt != want) { napi_throw_type_error(env, nullptr, "samples must be the format's typed array: Float32Array, Int16Array or (G.711) Uint8Array"); return nullptr; }
    if (pitch < cols || need > olen) { napi_throw_range_error(env, nullptr, "samples too short"); return nullptr; }
  }
  napi_value len_v = make_typed(env, napi_uint32_array, S, 4, &olens);
  if (!len_v) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  int rc = fskhip_modulate_host_fmt(e, (const uint8_t *)pdata, (const uint32_t *)ldata, ppitch, format, layout, out, n, pitch, (uint32_t *)olens);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value res;
  NAPI_OK(napi_create_object(env, &res));
  napi_set_named_property(env, res, "out", out_v);
  napi_set_named_property(env, res, "lens", len_v);
  return res;
}

static napi_value ModulatedLength(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  napi_value r;
  napi_create_double(env, (double)fskhip_modulated_length(e, u32(env, argv[1])), &r);
  return r;
}

static napi_value Reset(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  int64_t s = -1;
  napi_get_value_int64(env, argv[1], &s);
  int rc = fskhip_reset(e, s);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// carryOver(dst, src): what FSKCore.configure() leaves in place on a configured instance (fskhip_carry_over)
static napi_value CarryOver(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  fskhip_engine *dst = get_engine(env, argv[0]);
  if (!dst) return nullptr;
  fskhip_engine *src = get_engine(env, argv[1]);
  if (!src) return nullptr;
  int rc = fskhip_carry_over(dst, src);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// remapStreams(dst, src, map): stream i of dst continues stream map[i] of src, or starts afresh where map[i] is -1
// (fskhip_remap_streams); map is an Array of integers, one per stream of dst
static napi_value RemapStreams(napi_env env, napi_callback_info info) {
  ARGS_UPTO(3);
  fskhip_engine *dst = get_engine(env, argv[0]);
  if (!dst) return nullptr;
  fskhip_engine *src = get_engine(env, argv[1]);
  if (!src) return nullptr;
  std::vector<int64_t> map;
  if (!index_array(env, argv[2], "remapStreams: map must be an Array of stream indices (-1: a new stream)", &map, "remapStreams: map entries must be integers")) return nullptr;
  int rc = fskhip_remap_streams(dst, src, map.data(), (uint32_t)map.size());
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// ---- stream snapshots (include/fskhip.h): a snapshot is a Buffer (or any Uint8Array) on this side
static bool get_blob(napi_env env, napi_value v, const void **data, size_t *size) {
  bool is = false;
  void *p = nullptr;
  if (napi_is_buffer(env, v, &is) == napi_ok && is && napi_get_buffer_info(env, v, &p, size) == napi_ok) { *data = p; return true; }
  if (napi_is_typedarray(env, v, &is) == napi_ok && is) {
    napi_typedarray_type t;
    size_t n = 0;
    if (napi_get_typedarray_info(env, v, &t, &n, &p, nullptr, nullptr) == napi_ok && t == napi_uint8_array) { *data = p; *size = n; return true; }
  }
  napi_throw_type_error(env, nullptr, "a snapshot must be a Buffer or Uint8Array");
  return false;
}

// snapshotStreams(handle, sel): Buffer with streams sel (an Array of stream indices; null / undefined: all, in order)
static napi_value SnapshotStreams(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  fskhip_engine *e = argc >= 1 ? get_engine(env, argv[0]) : nullptr;
  if (!e) { if (argc < 1) napi_throw_type_error(env, nullptr, "snapshotStreams(handle, sel)"); return nullptr; }
  std::vector<int64_t> sel;
  const bool all = nullish(env, argv[1]);
  if (!all && !index_array(env, argv[1], "snapshotStreams: sel must be an Array of stream indices", &sel)) return nullptr;
  const uint32_t n = all ? fskhip_n_streams(e) : (uint32_t)sel.size();
  const size_t need = fskhip_snapshot_bytes(e, n);
  void *data = nullptr;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, need, &data, &buf));
  const int rc = fskhip_snapshot_streams(e, index_data(sel, all), n, data, need, nullptr);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return buf;
}

// restoreStreams(dst, snapshot, map): stream i of dst continues record map[i] of the snapshot, or starts afresh where map[i] is -1
static napi_value RestoreStreams(napi_env env, napi_callback_info info) {
  ARGS_UPTO(3);
  if (argc < 3) { napi_throw_type_error(env, nullptr, "restoreStreams(dst, snapshot, map)"); return nullptr; }
  fskhip_engine *dst = get_engine(env, argv[0]);
  if (!dst) return nullptr;
  const void *data = nullptr;
  size_t size = 0;
  if (!get_blob(env, argv[1], &data, &size)) return nullptr;
  std::vector<int64_t> map;
  if (!index_array(env, argv[2], "restoreStreams: map must be an Array of record indices (-1: a new stream)", &map)) return nullptr;
  const int rc = fskhip_restore_streams(dst, data, size, map.data(), (uint32_t)map.size());
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}

// snapshotInfo(snapshot) -> {nStreams, precision, perStreamConfigs, recordBytes, demodulationCalls, totalSamplesProcessed}
static napi_value SnapshotInfo(napi_env env, napi_callback_info info) {
  ARGS_UPTO(1);
  const void *data = nullptr;
  size_t size = 0;
  if (argc < 1 || !get_blob(env, argv[0], &data, &size)) { if (argc < 1) napi_throw_type_error(env, nullptr, "snapshotInfo(snapshot)"); return nullptr; }
  fskhip_snapshot_info si;
  const int rc = fskhip_snapshot_info_get(data, size, &si);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  set_num(env, o, "nStreams", si.n_streams);
  set_num(env, o, "precision", si.precision);
  set_num(env, o, "perStreamConfigs", si.per_stream_configs);
  set_num(env, o, "recordBytes", si.record_bytes);
  set_num(env, o, "demodulationCalls", si.demodulationCalls);
  set_num(env, o, "totalSamplesProcessed", si.totalSamplesProcessed);
  return o;
}

// snapshotConfig(snapshot, i) -> the FSKConfig record i ran under
static napi_value SnapshotConfig(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  const void *data = nullptr;
  size_t size = 0;
  if (argc < 2 || !get_blob(env, argv[0], &data, &size)) { if (argc < 2) napi_throw_type_error(env, nullptr, "snapshotConfig(snapshot, i)"); return nullptr; }
  uint32_t i = 0;
  NAPI_OK(napi_get_value_uint32(env, argv[1], &i));
  fskhip_config c;
  const int rc = fskhip_snapshot_stream_config(data, size, i, &c);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o, arr, v;
  NAPI_OK(napi_create_object(env, &o));
  set_num(env, o, "sampleRate", c.sampleRate); set_num(env, o, "baudRate", c.baudRate);
  set_num(env, o, "markFrequency", c.markFrequency); set_num(env, o, "spaceFrequency", c.spaceFrequency);
  set_num(env, o, "startBits", c.startBits); set_num(env, o, "stopBits", c.stopBits);
  set_num(env, o, "syncThreshold", c.syncThreshold); set_num(env, o, "preFilterBandwidth", c.preFilterBandwidth);
  NAPI_OK(napi_create_array_with_length(env, (size_t)c.preambleLen, &arr));
  for (int32_t k = 0; k < c.preambleLen; k++) { napi_create_int32(env, c.preamblePattern[k], &v); napi_set_element(env, arr, (uint32_t)k, v); }
  napi_set_named_property(env, o, "preamblePattern", arr);
  NAPI_OK(napi_create_array_with_length(env, (size_t)c.sfdLen, &arr));
  for (int32_t k = 0; k < c.sfdLen; k++) { napi_create_int32(env, c.sfdPattern[k], &v); napi_set_element(env, arr, (uint32_t)k, v); }
  napi_set_named_property(env, o, "sfdPattern", arr);
  const char *par = c.parity == 1 ? "even" : c.parity == 2 ? "odd" : "none";
  napi_create_string_utf8(env, par, NAPI_AUTO_LENGTH, &v);
  napi_set_named_property(env, o, "parity", v);
  set_bool(env, o, "agcEnabled", c.agcEnabled != 0);
  set_bool(env, o, "adaptiveThreshold", c.adaptiveThreshold != 0);
  return o;
}

// snapshotConcat([snapshot, ...]) -> Buffer: the records of all of them under one header (images of what could have been one engine)
static napi_value SnapshotConcat(napi_env env, napi_callback_info info) {
  ARGS_UPTO(1);
  bool is_arr = false;
  if (argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) { napi_throw_type_error(env, nullptr, "snapshotConcat: an Array of snapshots"); return nullptr; }
  uint32_t n = 0;
  NAPI_OK(napi_get_array_length(env, argv[0], &n));
  std::vector<const void *> ptrs(n);
  std::vector<size_t> sizes(n);
  for (uint32_t k = 0; k < n; k++) {
    napi_value v;
    NAPI_OK(napi_get_element(env, argv[0], k, &v));
    if (!get_blob(env, v, &ptrs[k], &sizes[k])) return nullptr;
  }
  size_t need = 0;
  int rc = fskhip_snapshot_concat(ptrs.data(), sizes.data(), n, nullptr, 0, &need);
  if (rc != FSKHIP_E_OVERFLOW) return throw_fsk(env, rc);
  void *data = nullptr;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, need, &data, &buf));
  rc = fskhip_snapshot_concat(ptrs.data(), sizes.data(), n, data, need, nullptr);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return buf;
}

// enableSignalQuality(handle, on) / getSignalQualityEstimates(handle, stream): the opt-in estimates of include/fskhip.h
static napi_value EnableSignalQuality(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  bool on = true;
  if (argc > 1) napi_get_value_bool(env, argv[1], &on);
  int rc = fskhip_enable_signal_quality(e, on ? 1 : 0);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  return nullptr;
}
static napi_value GetSignalQualityEstimates(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  fskhip_signal_quality q;
  int rc = fskhip_get_signal_quality(e, u32(env, argv[1]), &q);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  set_num(env, obj, "snr", q.snr); set_num(env, obj, "ber", q.ber); set_num(env, obj, "eyeOpening", q.eyeOpening);
  set_num(env, obj, "phaseJitter", q.phaseJitter); set_num(env, obj, "frequencyOffset", q.frequencyOffset);
  set_num(env, obj, "signalLevel", q.signalLevel); set_num(env, obj, "noiseFloor", q.noiseFloor);
  set_num(env, obj, "frames", q.frames); set_num(env, obj, "bytes", q.bytes);
  return obj;
}

// getStatus() (fsk.ts:481-493)
static napi_value GetStatus(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  fskhip_status st;
  int rc = fskhip_get_status(e, u32(env, argv[1]), &st);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  napi_value o;
  NAPI_OK(napi_create_object(env, &o));
  set_bool(env, o, "ready", st.ready != 0);
  set_bool(env, o, "frameStarted", st.frameStarted != 0);
  set_num(env, o, "globalSampleCounter", st.globalSampleCounter);
  set_num(env, o, "receivedBitsLength", st.receivedBitsLength);
  set_num(env, o, "byteBufferLength", st.byteBufferLength);
  set_num(env, o, "demodulationCalls", st.demodulationCalls);
  set_num(env, o, "syncDetections", st.syncDetections);
  set_num(env, o, "silenceThreshold", st.silenceThreshold);
  set_num(env, o, "totalSamplesProcessed", st.totalSamplesProcessed);
  set_num(env, o, "agcGain", st.agcGain);
  set_num(env, o, "eodCount", st.eodCount);
  return o;
}

// getFaults(handle) -> Uint8Array[nStreams]: 1 = the stream's filter state is no longer finite (include/fskhip.h, fskhip_get_faults)
static napi_value GetFaults(napi_env env, napi_callback_info info) {
  ARGS_UPTO(2);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  const uint32_t n = u32(env, argv[1]);
  void *data = nullptr;
  napi_value ab, arr;
  NAPI_OK(napi_create_arraybuffer(env, n, &data, &ab));
  int rc = fskhip_get_faults(e, n ? static_cast<uint8_t *>(data) : nullptr, nullptr);
  if (rc != FSKHIP_OK) return throw_fsk(env, rc);
  NAPI_OK(napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &arr));
  return arr;
}

static napi_value DemodSupported(napi_env env, napi_callback_info info) {
  ARGS_UPTO(1);
  fskhip_engine *e = get_engine(env, argv[0]);
  if (!e) return nullptr;
  napi_value r;
  napi_get_boolean(env, fskhip_demod_supported(e) != 0, &r);
  return r;
}

static napi_value DeviceCount(napi_env env, napi_callback_info) {
  napi_value r;
  napi_create_int32(env, fskhip_device_count(), &r);
  return r;
}

napi_value InitNext(napi_env env, napi_value exports);  // fsk_addon_next.cc: include/fskhip_next.h

static napi_value Init(napi_env env, napi_value exports) {
  const napi_property_descriptor props[] = {
      {"create", nullptr, Create, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"destroy", nullptr, Destroy, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"demodulate", nullptr, Demodulate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"demodulateAsync", nullptr, DemodulateAsync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"demodulateSamples", nullptr, DemodulateSamples, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"demodulateSamplesAsync", nullptr, DemodulateSamplesAsync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"modulateSamples", nullptr, ModulateSamples, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"modulate", nullptr, Modulate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"modulatedLength", nullptr, ModulatedLength, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"reset", nullptr, Reset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"carryOver", nullptr, CarryOver, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"remapStreams", nullptr, RemapStreams, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"snapshotStreams", nullptr, SnapshotStreams, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"restoreStreams", nullptr, RestoreStreams, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"snapshotInfo", nullptr, SnapshotInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"snapshotConfig", nullptr, SnapshotConfig, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"snapshotConcat", nullptr, SnapshotConcat, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"enableSignalQuality", nullptr, EnableSignalQuality, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getSignalQualityEstimates", nullptr, GetSignalQualityEstimates, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getStatus", nullptr, GetStatus, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getFaults", nullptr, GetFaults, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"demodSupported", nullptr, DemodSupported, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"deviceCount", nullptr, DeviceCount, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  napi_value v;
  napi_create_int32(env, fskhip_abi_version(), &v);
  napi_set_named_property(env, exports, "abiVersion", v);
  return InitNext(env, exports);
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
