// addon_util.h -- what the entry points of fsk_addon.cc and fsk_addon_next.cc are spelled with: the argument prologue, the
// unchecked numeric reads, typed arrays in and out, index lists, result-object setters, and the throw that carries the C
// library's message.  Everything is static: the two files share the text, not the symbols.
#pragma once
#include <node_api.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/fskhip.h"

#define NAPI_OK(call)                                                        \
  do {                                                                       \
    if ((call) != napi_ok) {                                                 \
      napi_throw_error(env, nullptr, "N-API call failed: " #call);           \
      return nullptr;                                                        \
    }                                                                        \
  } while (0)

// the first n arguments as argv[0 .. n) (those not passed are `undefined`), argc as passed
#define ARGS_UPTO(n)                                                         \
  size_t argc = n;                                                           \
  napi_value argv[n];                                                        \
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr))
// ... of an entry point that refuses fewer
#define ARGS(n)                                                              \
  ARGS_UPTO(n);                                                              \
  if (argc < n) { napi_throw_type_error(env, nullptr, "too few arguments"); return nullptr; }

static inline napi_value throw_fsk(napi_env env, int rc) {
  char code[16];
  snprintf(code, sizeof(code), "%d", rc);
  napi_throw_error(env, code, fskhip_last_error());
  return nullptr;
}

// numbers as JS converts them; what is no number reads as 0
static inline uint32_t u32(napi_env env, napi_value v) { uint32_t x = 0; napi_get_value_uint32(env, v, &x); return x; }
static inline int32_t i32(napi_env env, napi_value v) { int32_t x = 0; napi_get_value_int32(env, v, &x); return x; }
static inline double f64(napi_env env, napi_value v) { double x = 0; napi_get_value_double(env, v, &x); return x; }

static inline bool nullish(napi_env env, napi_value v) {
  napi_valuetype vt = napi_undefined;
  napi_typeof(env, v, &vt);
  return vt == napi_null || vt == napi_undefined;
}
static inline void *external(napi_env env, napi_value v, const char *what) {
  void *p = nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) { napi_throw_error(env, nullptr, what); return nullptr; }
  return p;
}

// a fresh typed array of `count` elements of `elem` bytes; *data is its storage
static inline napi_value make_typed(napi_env env, napi_typedarray_type t, size_t count, size_t elem, void **data) {
  napi_value ab, ta;
  if (napi_create_arraybuffer(env, count * elem, data, &ab) != napi_ok) return nullptr;
  if (napi_create_typedarray(env, t, count, ab, 0, &ta) != napi_ok) return nullptr;
  return ta;
}
// borrows a typed array of the given type; null/undefined -> data = nullptr when `optional`
static inline bool typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len, bool optional = false) {
  if (optional && nullish(env, v)) { *data = nullptr; *len = 0; return true; }
  bool is = false;
  napi_is_typedarray(env, v, &is);
  napi_typedarray_type tt;
  if (!is || napi_get_typedarray_info(env, v, &tt, len, data, nullptr, nullptr) != napi_ok || tt != want) {
    napi_throw_type_error(env, nullptr, "wrong typed array argument");
    return false;
  }
  return true;
}

// the capture formats (FSKHIP_SAMPLES_* / FSKHIP_LAYOUT_*): whether the pair is one (throws a TypeError where not), the typed array
// a format's samples come in, and the fill of a fresh G.711 array with the format's silence (the other formats' is the zero
// a fresh array holds)
static inline bool sample_format_ok(napi_env env, int32_t format, int32_t layout) {
  if (fskhip_sample_bytes(format) && (layout == FSKHIP_LAYOUT_STREAM_MAJOR || layout == FSKHIP_LAYOUT_SAMPLE_MAJOR)) return true;
  napi_throw_type_error(env, nullptr, "unknown sample format or layout");
  return false;
}
static inline napi_typedarray_type sample_array_type(int32_t format) {
  return format == FSKHIP_SAMPLES_F32 ? napi_float32_array : format == FSKHIP_SAMPLES_S16 ? napi_int16_array : napi_uint8_array;
}
static inline void fill_silence(int32_t format, void *out, size_t count) {
  if (format == FSKHIP_SAMPLES_MULAW || format == FSKHIP_SAMPLES_ALAW) memset(out, format == FSKHIP_SAMPLES_MULAW ? 0xFF : 0xD5, count);
}

// an Array of integers; throws `what` as a TypeError when it is no Array, `what_entry` (default: `what`) at an entry that is no integer
static inline bool index_array(napi_env env, napi_value arr, const char *what, std::vector<int64_t> *out, const char *what_entry = nullptr) {
  bool is_arr = false;
  if (napi_is_array(env, arr, &is_arr) != napi_ok || !is_arr) { napi_throw_type_error(env, nullptr, what); return false; }
  uint32_t n = 0;
  napi_get_array_length(env, arr, &n);
  out->resize(n);
  for (uint32_t i = 0; i < n; i++) {
    napi_value v;
    double d = 0;
    if (napi_get_element(env, arr, i, &v) != napi_ok || napi_get_value_double(env, v, &d) != napi_ok || d != (double)(int64_t)d) {
      napi_throw_type_error(env, nullptr, what_entry ? what_entry : what);
      return false;
    }
    (*out)[i] = (int64_t)d;
  }
  return true;
}
// the pointer the C calls take for an index list of v.size() entries: null means "all" to them, so an empty list still gets one
static inline const int64_t *index_data(const std::vector<int64_t> &v, bool all = false) {
  static const int64_t empty[1] = {0};
  return all ? nullptr : v.empty() ? empty : v.data();
}

static inline void set_num(napi_env env, napi_value obj, const char *k, double v) {
  napi_value n;
  napi_create_double(env, v, &n);
  napi_set_named_property(env, obj, k, n);
}
static inline void set_u32(napi_env env, napi_value obj, const char *k, uint32_t v) {
  napi_value n;
  napi_create_uint32(env, v, &n);
  napi_set_named_property(env, obj, k, n);
}
static inline void set_bool(napi_env env, napi_value obj, const char *k, bool v) {
  napi_value n;
  napi_get_boolean(env, v, &n);
  napi_set_named_property(env, obj, k, n);
}
