// fsk_host.h -- host-side helpers shared by the C-ABI translation units of libfskhip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fskhip.h"
#include "../../include/fskhip_next.h"

namespace fsk {
// records the thread-local message fskhip_last_error() returns and hands `code` back
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
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
