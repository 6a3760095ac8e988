// fsk_api.hip -- C ABI of libfskhip.so (include/fskhip.h): the error string, device selection (fsk_host.h), memory helpers, timing, the clock probe and the
// modulator / synthetic-signal entry points (the rest: fsk_create, fsk_options, fsk_dispatch, fsk_state).  No torch types, no CPU fallback.
#include <cmath>
#include <cstdarg>

#include "fsk_engine.h"
#include "fsk_launch.h"

using namespace fsk;

static thread_local std::string g_err;
int fsk::fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
int fsk::select_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FSKHIP_E_NO_DEVICE, "no HIP device available (the engine has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(FSKHIP_E_NO_DEVICE, "device %d out of range (%d devices)", device, ndev);
  if (hipSetDevice(device) != hipSuccess) return fail(FSKHIP_E_NO_DEVICE, "hipSetDevice(%d) failed", device);
  return FSKHIP_OK;
}

namespace {
// one wave: shader cycles (s_memtime) and 100 MHz ticks (s_memrealtime) across `ticks` of sleeping (include/fskhip.h)
__global__ void clock_probe_kernel(unsigned long long *out, unsigned long long ticks) {
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  unsigned long long r = r0;
  while (r - r0 < ticks) {
    __builtin_amdgcn_s_sleep(127);
    r = __builtin_amdgcn_s_memrealtime();
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r - r0; }
}
}  // namespace

// the bracket around one call's launches while timing is on (the demodulate and modulate entry points)
int fsk::timing_open(fskhip_engine *e, hipStream_t st) {
  fskhip_engine::Timing &t = e->timing;
  if (!t.on) return FSKHIP_OK;
  if (t.used + 2 > t.ev.size()) {
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    t.ev.push_back(a); t.ev.push_back(b);
  }
  t.stream = st;
  HIP_TRY(hipEventRecord(t.ev[t.used], st));
  return FSKHIP_OK;
}
int fsk::timing_close(fskhip_engine *e, hipStream_t st) {
  fskhip_engine::Timing &t = e->timing;
  if (!t.on) return FSKHIP_OK;
  HIP_TRY(hipEventRecord(t.ev[t.used + 1], st));
  t.used += 2;
  return FSKHIP_OK;
}

extern "C" {
const char *fskhip_last_error(void) { return g_err.c_str(); }
int fskhip_abi_version(void) { return FSKHIP_ABI_VERSION; }
int fskhip_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
// Page-locked host memory for the _host entry points (so that their H2D / D2H copies run asynchronously at full PCIe
// rate); plain hipHostMalloc / hipHostFree for hosts without a HIP binding of their own.
int fskhip_host_alloc(size_t bytes, void **ptr) {
  if (!ptr) return fail(FSKHIP_E_INVALID, "null pointer");
  *ptr = nullptr;
  hipError_t err = hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault);
  if (err != hipSuccess) return fail(err == hipErrorNoDevice ? FSKHIP_E_NO_DEVICE : FSKHIP_E_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(err));
  return FSKHIP_OK;
}
int fskhip_host_free(void *ptr) {
  if (ptr) HIP_TRY(hipHostFree(ptr));
  return FSKHIP_OK;
}
size_t fskhip_modulated_length(const fskhip_engine *e, size_t n_bytes) {  // fsk.ts:391-394
  if (!e) return 0;
  const double total_bytes = (double)e->cfg0.preambleLen + (double)e->cfg0.sfdLen + (double)n_bytes;
  const double padding = total_bytes > 0 ? e->spb * 2 : 0;
  const double silence = e->bpb * e->spb;
  return (size_t)(total_bytes * e->bpb * e->spb + padding + silence);
}
int fskhip_modulate_device(fskhip_engine *e, const uint8_t *d_payloads, const uint32_t *d_lens, size_t payload_pitch,
                           float *d_out, size_t out_pitch, uint32_t *d_out_lens, void *hip_stream) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "FSK modulator not configured");
  if (!d_lens || !d_out || !d_out_lens) return fail(FSKHIP_E_INVALID, "null buffer");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)hip_stream;
  if (const int rc = timing_open(e, st)) return rc;     // (fskhip_timing_begin / _end bracket modulate launches too: bench.py --workload mod)
  HIP_TRY(launch_modulate(e->M, e->S.coef, d_payloads, d_lens, payload_pitch, d_out, out_pitch, d_out_lens, st));
  if (const int rc = timing_close(e, st)) return rc;
  return FSKHIP_OK;
}
int fskhip_modulate_host(fskhip_engine *e, const uint8_t *payloads, const uint32_t *lens, size_t payload_pitch,
                         float *out, size_t out_pitch, uint32_t *out_lens) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "FSK modulator not configured");
  if (!lens || !out || !out_lens) return fail(FSKHIP_E_INVALID, "null buffer");
  HIP_TRY(hipSetDevice(e->device));
  const size_t S = e->n_streams;
  const size_t dpitch = (out_pitch + 3) & ~(size_t)3;
  int rc;
  if ((rc = ensure(e->host.d_samples, e->host.d_samples_cap, (dpitch ? dpitch : 4) * S)) != FSKHIP_OK) return rc;
  if ((rc = ensure(e->host.d_payloads, e->host.d_payloads_cap, (payload_pitch ? payload_pitch : 1) * S)) != FSKHIP_OK) return rc;
  for (size_t s = 0; s < S; s++)
    if (lens[s] > payload_pitch) return fail(FSKHIP_E_INVALID, "lens[%zu] = %u exceeds payload_pitch %zu", s, lens[s], payload_pitch);
  if (payload_pitch > 0 && payloads)
    HIP_TRY(hipMemcpyAsync(e->host.d_payloads, payloads, payload_pitch * S, hipMemcpyHostToDevice, e->host.stream));
  HIP_TRY(hipMemcpyAsync(e->host.d_lens, lens, sizeof(uint32_t) * S, hipMemcpyHostToDevice, e->host.stream));
  rc = fskhip_modulate_device(e, e->host.d_payloads, e->host.d_lens, payload_pitch, e->host.d_samples, dpitch, e->host.d_counts, e->host.stream);
  if (rc != FSKHIP_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_lens, e->host.d_counts, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, e->host.stream));
  HIP_TRY(hipMemcpy2DAsync(out, out_pitch * sizeof(float), e->host.d_samples, dpitch * sizeof(float),
                           out_pitch * sizeof(float), S, hipMemcpyDeviceToHost, e->host.stream));
  HIP_TRY(hipStreamSynchronize(e->host.stream));
  if (const int hrc = handoff_check(e, true)) return hrc;
  for (size_t s = 0; s < S; s++)
    if (out_lens[s] > out_pitch) return fail(FSKHIP_E_OVERFLOW, "stream %zu needs %u samples, slab holds %zu", s, out_lens[s], out_pitch);
  return FSKHIP_OK;
}
// ... and the same into any capture format and layout (include/fskhip.h): the floats stay on the device, fsk_samples.hip's egress kernel narrows
// them -- silence from the modulator's own d_out_lens on -- into a staging buffer kept with the engine, and the narrow samples cross
// PCIe in one 2-D copy: rows of n elements (stream-major), or n frames of n_streams elements (sample-major: the staging frames are
// packed, the caller's may be wider and keep their other columns)
int fskhip_modulate_host_fmt(fskhip_engine *e, const uint8_t *payloads, const uint32_t *lens, size_t payload_pitch, int format, int layout, void *out, size_t n,
                             size_t dst_pitch, uint32_t *out_lens) {
  if (const int rc = check_sample_format("fskhip_modulate_host_fmt", format, layout)) return rc;
  const size_t esz = sample_bytes(format);
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "FSK modulator not configured");
  if (!lens || !out_lens || (n > 0 && !out)) return fail(FSKHIP_E_INVALID, "null buffer");
  const size_t S = e->n_streams;
  const bool frames = layout == FSKHIP_LAYOUT_SAMPLE_MAJOR;
  if (!frames && dst_pitch < n) return fail(FSKHIP_E_INVALID, "dst_pitch %zu < n_per_stream %zu", dst_pitch, n);
  if (frames && dst_pitch < S) return fail(FSKHIP_E_INVALID, "frame pitch %zu < n_streams %zu", dst_pitch, S);
  if ((reinterpret_cast<uintptr_t>(out) & (esz - 1u)) != 0) return fail(FSKHIP_E_INVALID, "out is not aligned to its element size");
  for (size_t s = 0; s < S; s++)
    if (lens[s] > payload_pitch) return fail(FSKHIP_E_INVALID, "lens[%zu] = %u exceeds payload_pitch %zu", s, lens[s], payload_pitch);
  HIP_TRY(hipSetDevice(e->device));
  const EgressStage g = egress_stage(S, n, esz, frames);
  int rc;
  if ((rc = ensure(e->host.d_samples, e->host.d_samples_cap, (g.fpitch ? g.fpitch : 4) * S)) != FSKHIP_OK) return rc;
  if ((rc = ensure(e->host.d_payloads, e->host.d_payloads_cap, (payload_pitch ? payload_pitch : 1) * S)) != FSKHIP_OK) return rc;
  if (n > 0 && (rc = ensure(e->host.d_egress, e->host.d_egress_cap, g.bytes)) != FSKHIP_OK) return rc;
  if (payload_pitch > 0 && payloads)
    HIP_TRY(hipMemcpyAsync(e->host.d_payloads, payloads, payload_pitch * S, hipMemcpyHostToDevice, e->host.stream));
  HIP_TRY(hipMemcpyAsync(e->host.d_lens, lens, sizeof(uint32_t) * S, hipMemcpyHostToDevice, e->host.stream));
  rc = fskhip_modulate_device(e, e->host.d_payloads, e->host.d_lens, payload_pitch, e->host.d_samples, g.fpitch, e->host.d_counts, e->host.stream);
  if (rc != FSKHIP_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_lens, e->host.d_counts, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, e->host.stream));
  if (n > 0) {
    const hipError_t err = launch_egress(e->host.d_samples, g.fpitch, e->host.d_counts, (uint32_t)S, n, format, layout, e->host.d_egress, g.npitch, e->host.stream);
    if (err == hipErrorInvalidValue) return fail(FSKHIP_E_INVALID, "fskhip_modulate_host_fmt: %zu streams x %zu samples are more workgroups than one launch takes", S, n);
    HIP_TRY(err);
    HIP_TRY(hipMemcpy2DAsync(out, dst_pitch * esz, e->host.d_egress, g.npitch * esz, g.row_bytes, g.rows, hipMemcpyDeviceToHost, e->host.stream));
  }
  HIP_TRY(hipStreamSynchronize(e->host.stream));
  if (const int hrc = handoff_check(e, true)) return hrc;
  for (size_t s = 0; s < S; s++)
    if (out_lens[s] > n) return fail(FSKHIP_E_OVERFLOW, "stream %zu needs %u samples, slab holds %zu", s, out_lens[s], n);
  return FSKHIP_OK;
}
int fskhip_synth_device(fskhip_engine *e, float *d_out, size_t n, size_t pitch, uint32_t payload_len, uint64_t seed,
                        uint32_t lead_max, double amp_lo, double amp_hi, void *hip_stream) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "not configured");
  if (!d_out || pitch < n) return fail(FSKHIP_E_INVALID, "bad buffer");
  if (n == 0) return FSKHIP_OK;  // nothing to write: no launch
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(launch_synth(e->M, e->S.coef, d_out, n, pitch, payload_len, seed, lead_max, amp_lo, amp_hi,
                       (hipStream_t)hip_stream));
  return FSKHIP_OK;
}
uint8_t fskhip_synth_payload_byte(uint64_t seed, uint32_t stream, uint32_t frame, uint32_t i) {
  return host_synth_payload_byte(seed, stream, frame, i);
}
void fskhip_synth_stream_params(uint64_t seed, uint32_t stream, uint32_t lead_max, double amp_lo, double amp_hi,
                                uint32_t *lead, double *amp) {
  host_synth_stream_params(seed, stream, lead_max, amp_lo, amp_hi, lead, amp);
}
int fskhip_add_awgn_device(fskhip_engine *e, float *d_buf, size_t n, size_t pitch, double snr_db, uint64_t seed,
                           void *hip_stream) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "not configured");
  if (!d_buf || pitch < n) return fail(FSKHIP_E_INVALID, "bad buffer");
  if (!std::isfinite(snr_db)) return fail(FSKHIP_E_INVALID, "fskhip_add_awgn_device: snr_db is not finite");
  if (n == 0) return FSKHIP_OK;  // nothing to noise: a zero-wide grid is no launch HIP takes
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(launch_awgn(d_buf, n, pitch, e->n_streams, snr_db, seed, e->d_sigma, (hipStream_t)hip_stream));
  return FSKHIP_OK;
}
int fskhip_probe_read_device(fskhip_engine *e, const float *d_buf, size_t n, size_t pitch, void *hip_stream) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "not configured");
  if (!d_buf || pitch < n || (pitch % 4) != 0) return fail(FSKHIP_E_INVALID, "bad buffer");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(launch_probe_read(d_buf, n, pitch, e->n_streams, (float *)e->d_sigma, (hipStream_t)hip_stream));
  return FSKHIP_OK;
}
int fskhip_device_malloc(fskhip_engine *e, size_t bytes, void **d_ptr) {
  if (!e || !d_ptr) return fail(FSKHIP_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  hipError_t err = hipMalloc(d_ptr, bytes ? bytes : 1);
  if (err != hipSuccess) return fail(FSKHIP_E_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(err));
  return FSKHIP_OK;
}
int fskhip_device_free(fskhip_engine *e, void *d_ptr) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipFree(d_ptr));
  return FSKHIP_OK;
}
int fskhip_memcpy_h2d(fskhip_engine *e, void *d_dst, const void *src, size_t bytes) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
  return FSKHIP_OK;
}
int fskhip_memcpy_d2h(fskhip_engine *e, void *dst, const void *d_src, size_t bytes) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}
int fskhip_synchronize(fskhip_engine *e) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  return handoff_check(e, true);
}
int fskhip_clock_probe_begin(fskhip_engine *e, double spin_ms) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  if (!(spin_ms > 0) || spin_ms > 10000.0) return fail(FSKHIP_E_INVALID, "spin_ms %g out of range (0, 10000]", spin_ms);
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_clock) HIP_TRY(hipMalloc((void **)&e->d_clock, 2 * sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(e->d_clock, 0, 2 * sizeof(unsigned long long), e->host.stream));
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, e->host.stream, e->d_clock, (unsigned long long)(spin_ms * 1.0e5));
  HIP_TRY(hipGetLastError());
  return FSKHIP_OK;
}
int fskhip_clock_probe_end(fskhip_engine *e, double *shader_ghz, double *covered_ms) {
  if (!e || !e->d_clock) return fail(FSKHIP_E_INVALID, "no clock probe in flight");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->host.stream));
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpy(h, e->d_clock, sizeof(h), hipMemcpyDeviceToHost));
  if (!h[1]) return fail(FSKHIP_E_HIP, "clock probe returned no ticks");
  if (shader_ghz) *shader_ghz = (double)h[0] / (double)h[1] * 0.1;
  if (covered_ms) *covered_ms = (double)h[1] * 1.0e-5;
  return FSKHIP_OK;
}
int fskhip_timing_begin(fskhip_engine *e) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  e->timing.on = true;
  e->timing.used = 0;
  return FSKHIP_OK;
}
int fskhip_timing_end(fskhip_engine *e, uint32_t *n_launches, double *total_ms) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  e->timing.on = false;
  double tot = 0;
  uint32_t n = 0;
  for (size_t i = 0; i + 1 < e->timing.used; i += 2) {
    HIP_TRY(hipEventSynchronize(e->timing.ev[i + 1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->timing.ev[i], e->timing.ev[i + 1]));
    tot += ms;
    n++;
  }
  e->timing.used = 0;
  if (n_launches) *n_launches = n;
  if (total_ms) *total_ms = tot;
  return FSKHIP_OK;
}
}  // extern "C"
