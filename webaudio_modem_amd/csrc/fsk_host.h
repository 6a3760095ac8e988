// fsk_host.h -- host-side helpers shared by the C-ABI translation units of libfskhip.so (not part of the ABI): the error
// string (fail; open_image for a flaw that a host-only image validator names), device selection, device allocation (dev_alloc,
// ensure for scratch that grows, Scratch for what lives as long as one call), the HIP_TRY macros and, behind them, the per-stream
// word arrays of the resident XModem handles (fill_words, get_words, put_words).  What only some units share lives beside them:
// fsk_filter_host.h (the two filters' handles and _host calls), fsk_stage.h (the snapshot units' selection and room checks
// and slab pipelines; the image formats and their one frame are host-only: fsk_image.h), fsk_proc.h (struct fskhip_processor).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/fskhip.h"
#include "../../include/fskhip_next.h"

namespace fsk {
// records the thread-local message fskhip_last_error() returns and hands `code` back
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// opens an image with its format's host-only validator (fsk_*_image.h: xx_image_open); a flaw is the entry point's refusal
template <class Open, class Image>
int open_image(const char *who, Open open, const void *buf, size_t size, Image *im) {
  char msg[512];
  if (open(buf, size, im, msg, sizeof(msg))) return fail(FSKHIP_E_INVALID, "%s: %s", who, msg);
  return FSKHIP_OK;
}
// makes `device` current for a create call or a handle-less _host call: FSKHIP_E_NO_DEVICE where there is no device, the index
// is out of range or hipSetDevice refuses it (fsk_api.hip)
int select_device(int device);
// a device buffer of n elements (of one where n is 0)
template <typename T>
int dev_alloc(T *&p, size_t n) {
  hipError_t err = hipMalloc((void **)&p, (n ? n : 1) * sizeof(T));
  if (err != hipSuccess) return fail(FSKHIP_E_NOMEM, "hipMalloc(%zu): %s", n * sizeof(T), hipGetErrorString(err));
  return FSKHIP_OK;
}
// a device scratch buffer that only grows: at least `need` elements (its old contents are not kept)
template <typename T>
int ensure(T *&p, size_t &cap, size_t need) {
  if (need <= cap) return FSKHIP_OK;
  if (p) (void)hipFree(p);
  p = nullptr; cap = 0;
  hipError_t err = hipMalloc((void **)&p, need * sizeof(T));
  if (err != hipSuccess) return fail(FSKHIP_E_NOMEM, "hipMalloc(%zu): %s", need * sizeof(T), hipGetErrorString(err));
  cap = need;
  return FSKHIP_OK;
}
}  // namespace fsk

// a HIP call; on failure: run `cleanup`, record "<call>: <HIP's message>" and return FSKHIP_E_NOMEM (only if `oom_code`) or FSKHIP_E_HIP
#define HIP_TRY_AS(expr, text, oom_code, cleanup)                                                                      \
  do {                                                                                                                 \
    hipError_t _e = (expr);                                                                                            \
    if (_e != hipSuccess) {                                                                                            \
      cleanup;                                                                                                         \
      return fsk::fail((oom_code) && _e == hipErrorOutOfMemory ? FSKHIP_E_NOMEM : FSKHIP_E_HIP, "%s: %s", text, hipGetErrorString(_e)); \
    }                                                                                                                  \
  } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(expr, #expr, false, (void)0)

namespace fsk {
// device scratch of one call, freed when the call returns (after the device has been synchronised)
struct Scratch {
  std::vector<void *> bufs;
  ~Scratch() {
    for (void *b : bufs) (void)hipFree(b);
  }
  template <typename T>
  int alloc(T *&p, size_t n) {
    const int rc = dev_alloc(p, n);
    if (rc == FSKHIP_OK) bufs.push_back(p);
    return rc;
  }
  template <typename T>
  int upload(T *&p, const T *host, size_t n) {
    if (const int rc = alloc(p, n)) return rc;
    if (n) HIP_TRY(hipMemcpy(p, host, sizeof(T) * n, hipMemcpyHostToDevice));
    return FSKHIP_OK;
  }
};

// per-stream uint32 words on the device, as the three resident XModem handles keep them: n words set to `value`; n words to the
// host; n words from the host (a null `host` leaves them as they are).  Synchronous copies on the null stream.
inline int fill_words(uint32_t *d, size_t n, uint32_t value) {
  if (!n) return FSKHIP_OK;
  if (value == 0u) { HIP_TRY(hipMemset(d, 0, sizeof(uint32_t) * n)); return FSKHIP_OK; }
  const std::vector<uint32_t> host(n, value);
  HIP_TRY(hipMemcpy(d, host.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  return FSKHIP_OK;
}
inline int get_words(std::vector<uint32_t> &host, const uint32_t *d, size_t n) {
  host.resize(n);
  if (n) HIP_TRY(hipMemcpy(host.data(), d, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}
inline int put_words(uint32_t *d, const uint32_t *host, size_t n) {
  if (n && host) HIP_TRY(hipMemcpy(d, host, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  return FSKHIP_OK;
}
}  // namespace fsk
