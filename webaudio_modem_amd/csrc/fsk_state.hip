// fsk_state.hip -- C ABI of libfskhip.so (include/fskhip.h): reading and resetting the per-stream state between calls --
// reset, status, faults, the opt-in signal-quality estimates, the one-stream trace and the raw state words.
#include <limits>

#include "fsk_engine.h"

using namespace fsk;

// ---- small device kernels for state management --------------------------------------------------
namespace {
struct StatusRaw {
  double agc_gain, sil_thr;
  uint32_t started, gsc, ring_len, sync_det, eod_total, ds_cnt;
};
static_assert(sizeof(StatusRaw) == kStatusRawBytes, "fskhip_create allocates d_status");

template <typename Real>
__global__ void status_kernel(DemodState S, uint32_t n, uint32_t s, StatusRaw *out) {
  const Real *rs = (const Real *)S.rs;
  out->agc_gain = (double)rs[(size_t)RF_agc_gain * n + s];
  out->sil_thr = (double)rs[(size_t)RF_sil_thr * n + s];
  out->started = S.is[(size_t)IF_started * n + s];
  out->gsc = S.is[(size_t)IF_gsc * n + s];
  out->ring_len = S.is[(size_t)IF_ring_len * n + s];
  out->sync_det = S.is[(size_t)IF_sync_det * n + s];
  out->eod_total = S.is[(size_t)IF_eod_total * n + s];
  out->ds_cnt = S.is[(size_t)IF_ds_cnt * n + s];
}

// fskhip_get_faults: a stream whose filter state has left the finite range -- the pre-filter (never reset, fsk.ts:175-188), the
// I/Q low-pass, the post filter.  Once a NaN is in the pre-filter's recurrence it stays, so the flag is sticky by itself.
template <typename Real>
__global__ void faults_kernel(DemodState S, uint32_t n, uint8_t *out, uint32_t *count) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const Real *rs = (const Real *)S.rs;
  const int fields[] = {RF_bp_y1, RF_bp_y2, RF_bp_x1, RF_li_y1, RF_lq_y1, RF_po_y1, RF_agc_gain};
  bool bad = false;
  for (int f : fields) {
    const Real v = rs[(size_t)f * n + s];
    bad = bad || !(fabs((double)v) < (sizeof(Real) == 4 ? 1.0e38 : 1.0e300));
  }
  out[s] = bad ? 1 : 0;
  if (bad) atomicAdd(count, 1u);
}

// reset() fsk.ts:464-469 = resetState() + syncSamplesBuffer.clear() (+ host-side counters).
// stream < 0: all streams.
template <typename Real>
__global__ void reset_kernel(DemodState S, uint32_t n, int64_t stream) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  if (stream >= 0 && (int64_t)s != stream) return;
  Real *rs = (Real *)S.rs;
  const int rz[] = {RF_li_x1, RF_li_x2, RF_li_y1, RF_li_y2, RF_lq_x1, RF_lq_x2, RF_lq_y1, RF_lq_y2,
                    RF_po_x1, RF_po_x2, RF_po_y1, RF_po_y2, RF_acc_i,  RF_acc_q,  RF_last_phase, RF_nco_phase};
  for (int f : rz) rs[(size_t)f * n + s] = (Real)0;
  rs[(size_t)RF_nco_c * n + s] = (Real)1.0; rs[(size_t)RF_nco_s * n + s] = (Real)0;
  const int iz[] = {IF_nco_lo, IF_nco_hi, IF_ds_cnt, IF_gsc, IF_cad_ctr, IF_sil_cnt, IF_started, IF_bit_acc,
                    IF_bit_reload, IF_byte_cur, IF_bit_pos, IF_ring_len, IF_sync_det};
  if (sizeof(Real) == 4) {
    // fp32 engines (free-running frame, fsk_params.h): the NCO restarts at 0, so the frame offset becomes minus the
    // frame's own phase, and lastPhase = 0 is that phase in the frame; filters and correction start from zero
    const uint64_t acc = ((uint64_t)S.is[(size_t)IF_nco_hi * n + s] << 32) | S.is[(size_t)IF_nco_lo * n + s];
    const uint64_t off = ((uint64_t)S.is[(size_t)IF_fr_hi * n + s] << 32) | S.is[(size_t)IF_fr_lo * n + s];
    const uint64_t fr0 = acc - off, noff = 0ull - fr0;
    S.is[(size_t)IF_fr_lo * n + s] = (uint32_t)noff;
    S.is[(size_t)IF_fr_hi * n + s] = (uint32_t)(noff >> 32);
    const int zz[] = {RF_zq_ai, RF_zq_aq, RF_zq_bi, RF_zq_bq, RF_zq_0i, RF_zq_0q, RF_zd_ix1, RF_zd_ix2, RF_zd_iy, RF_zd_iv,
                      RF_zd_qx1, RF_zd_qx2, RF_zd_qy, RF_zd_qv};
    for (int f : zz) rs[(size_t)f * n + s] = (Real)0;
    S.is[(size_t)IF_zr_dph * n + s] = kHandPairs;
    double r = (double)fr0 * 5.42101086242752217e-20 * 6.283185307179586476925;
    r = r > 3.14159265358979323846 ? r - 6.283185307179586476925 : r;
    for (int f : iz) S.is[(size_t)f * n + s] = 0u;
    rs[(size_t)RF_last_phase * n + s] = (Real)r;
  } else {
    for (int f : iz) S.is[(size_t)f * n + s] = 0u;
  }
  S.is[(size_t)IF_bit_wait * n + s] = kBigWait;
}

// real field `f` of stream `s`, fp32 or fp64 as the engine keeps it
int read_real(const fskhip_engine *e, int f, uint32_t s, double *out) {
  const char *at = (const char *)e->S.rs + engine_real_row(e, f) + (size_t)s * engine_real_bytes(e);
  float v = 0;
  const bool f64 = e->precision == FSKHIP_PRECISION_F64;
  HIP_TRY(hipMemcpy(f64 ? (void *)out : (void *)&v, at, engine_real_bytes(e), hipMemcpyDeviceToHost));
  if (!f64) *out = (double)v;
  return FSKHIP_OK;
}
}  // namespace

extern "C" {
int fskhip_reset(fskhip_engine *e, int64_t stream) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "not configured");
  if (stream >= (int64_t)e->n_streams) return fail(FSKHIP_E_INVALID, "stream out of range");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  dim3 g((e->n_streams + 255) / 256), b(256);
  if (e->precision == FSKHIP_PRECISION_F64) hipLaunchKernelGGL(reset_kernel<double>, g, b, 0, 0, e->S, e->n_streams, stream);
  else hipLaunchKernelGGL(reset_kernel<float>, g, b, 0, 0, e->S, e->n_streams, stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  if (stream < 0) {
    for (auto &v : e->base_calls) v = e->calls;
    for (auto &v : e->base_samples) v = e->total_samples;
    e->ds_parity = 0;  // every decimator restarts; ring positions stay as they were (see below)
  } else {
    e->base_calls[stream] = e->calls;
    e->base_samples[stream] = e->total_samples;
    // the other streams may sit mid-pair of the /2 decimator: from now on this stream pushes into its
    // rings at other instants than its neighbours, for good (ring positions are never re-aligned)
    if (e->n_streams > 1 && e->ds_parity) e->ds_uniform = false;
    // a one-stream engine: its only decimator has just restarted at a pair boundary (found by tools/soak.py: the
    // host kept believing in the odd phase and later handed a mid-pair stream to the whole-tile kernels)
    if (e->n_streams == 1) e->ds_parity = 0;
  }
  return FSKHIP_OK;
}
int fskhip_get_status(fskhip_engine *e, uint32_t stream, fskhip_status *st) {
  if (!st) return fail(FSKHIP_E_INVALID, "null status");
  std::memset(st, 0, sizeof(*st));
  if (!e) return FSKHIP_OK;  // unconfigured FSKCore: ready = false
  if (stream >= e->n_streams) return fail(FSKHIP_E_INVALID, "stream out of range");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  if (e->precision == FSKHIP_PRECISION_F64) hipLaunchKernelGGL(status_kernel<double>, dim3(1), dim3(1), 0, 0, e->S, e->n_streams, stream, (StatusRaw *)e->d_status);
  else hipLaunchKernelGGL(status_kernel<float>, dim3(1), dim3(1), 0, 0, e->S, e->n_streams, stream, (StatusRaw *)e->d_status);
  HIP_TRY(hipGetLastError());
  StatusRaw r;
  HIP_TRY(hipMemcpy(&r, e->d_status, sizeof(r), hipMemcpyDeviceToHost));
  st->ready = 1;
  st->frameStarted = r.started != 0;
  st->globalSampleCounter = r.gsc;
  st->receivedBitsLength = r.ring_len;
  st->byteBufferLength = 0;
  st->demodulationCalls = (double)(e->calls - e->base_calls[stream]);
  st->syncDetections = r.sync_det;
  st->silenceThreshold = r.sil_thr;
  st->totalSamplesProcessed = (double)(e->total_samples - e->base_samples[stream]);
  st->agcGain = e->P.agc_on ? r.agc_gain : std::numeric_limits<double>::quiet_NaN();
  st->eodCount = r.eod_total;
  return FSKHIP_OK;
}
// Which streams' filter state is no longer finite (include/fskhip.h).  out: n_streams bytes (host) or null; n_faulty: host or null.
int fskhip_get_faults(fskhip_engine *e, uint8_t *out, uint32_t *n_faulty) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "not configured");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  if (const int hrc = handoff_check(e, true)) return hrc;
  uint8_t *d_out = nullptr;
  uint32_t *d_n = nullptr;
  HIP_TRY(hipMalloc((void **)&d_out, e->n_streams));
  if (hipMalloc((void **)&d_n, sizeof(uint32_t)) != hipSuccess) { (void)hipFree(d_out); return fail(FSKHIP_E_NOMEM, "fskhip_get_faults"); }
  hipError_t err = hipMemset(d_n, 0, sizeof(uint32_t));
  if (err == hipSuccess) {
    const dim3 g((e->n_streams + 255) / 256), b(256);
    if (e->precision == FSKHIP_PRECISION_F64) hipLaunchKernelGGL(faults_kernel<double>, g, b, 0, 0, e->S, e->n_streams, d_out, d_n);
    else hipLaunchKernelGGL(faults_kernel<float>, g, b, 0, 0, e->S, e->n_streams, d_out, d_n);
    err = hipGetLastError();
  }
  uint32_t n = 0;
  if (err == hipSuccess) err = hipMemcpy(&n, d_n, sizeof(n), hipMemcpyDeviceToHost);
  if (err == hipSuccess && out) err = hipMemcpy(out, d_out, e->n_streams, hipMemcpyDeviceToHost);
  (void)hipFree(d_out); (void)hipFree(d_n);
  if (err != hipSuccess) return fail(FSKHIP_E_HIP, "fskhip_get_faults: %s", hipGetErrorString(err));
  if (n_faulty) *n_faulty = n;
  return FSKHIP_OK;
}

// ---- opt-in signal-quality estimates (the definition is in include/fskhip.h) ----------------
int fskhip_enable_signal_quality(fskhip_engine *e, int on) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "not configured");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t n = e->n_streams;
  if (on) {   // the accumulators are contiguous rows at the end of both state arrays
    HIP_TRY(hipMemset((char *)e->S.rs + engine_real_row(e, RF_q_signal), 0, engine_real_row(e, RF_COUNT) - engine_real_row(e, RF_q_signal)));
    HIP_TRY(hipMemset(e->S.is + (size_t)IF_q_armed * n, 0, (size_t)(IF_COUNT - IF_q_armed) * n * sizeof(uint32_t)));
  }
  e->P.quality = on ? 1u : 0u;
  return FSKHIP_OK;
}
int fskhip_get_signal_quality(fskhip_engine *e, uint32_t stream, fskhip_signal_quality *q) {
  if (!q) return fail(FSKHIP_E_INVALID, "null result");
  std::memset(q, 0, sizeof(*q));
  if (!e) return FSKHIP_OK;                       // unconfigured FSKCore: the reference's zeros
  if (stream >= e->n_streams) return fail(FSKHIP_E_INVALID, "stream out of range");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t n = e->n_streams;
  double rv[RF_COUNT - RF_q_signal];
  uint32_t iv[IF_COUNT - IF_q_armed];
  for (int f = RF_q_signal; f < RF_COUNT; f++)
    if (const int rc = read_real(e, f, stream, &rv[f - RF_q_signal])) return rc;
  for (int f = IF_q_armed; f < IF_COUNT; f++)
    HIP_TRY(hipMemcpy(&iv[f - IF_q_armed], e->S.is + (size_t)f * n + stream, sizeof(uint32_t), hipMemcpyDeviceToHost));
#define QR(name) rv[RF_##name - RF_q_signal]
#define QI(name) ((double)iv[IF_##name - IF_q_armed])
  q->frames = QI(q_frames); q->bytes = QI(q_bytes);
  q->signalLevel = QR(q_signal); q->noiseFloor = QR(q_floor);
  if (QI(q_frames) > 0) q->snr = QR(q_floor) > 0 ? std::fmin(200.0, 20.0 * std::log10(QR(q_signal) / QR(q_floor))) : 200.0;
  if (QI(q_votes) > 0) q->ber = QI(q_minor) / QI(q_votes);
  if (QI(q_bytes) > 0) q->eyeOpening = QR(q_eye_sum) / QI(q_bytes);
  if (QI(q_ftrans) > 0) {
    const double m = QR(q_f_sum) / QI(q_ftrans), v = QR(q_f2_sum) / QI(q_ftrans) - m * m;
    q->phaseJitter = std::sqrt(v > 0 ? v : 0.0);
    if (QI(q_starts) > 0)
      q->frequencyOffset = -0.5 * (m + QR(q_f0_sum) / QI(q_starts)) * (e->cfg0.sampleRate / 2.0) / (2.0 * 3.14159265358979323846);
  }
#undef QR
#undef QI
  return FSKHIP_OK;
}
int fskhip_trace_enable(fskhip_engine *e, int64_t stream, size_t capacity) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  void *old[] = {e->S.trace_amp, e->S.trace_post, e->S.trace_bit, e->S.trace_n};
  for (void *b : old)
    if (b) (void)hipFree(b);
  e->S.trace_amp = nullptr; e->S.trace_post = nullptr; e->S.trace_bit = nullptr; e->S.trace_n = nullptr;
  e->S.trace_stream = 0xFFFFFFFFu; e->S.trace_cap = 0; e->trace_cap = 0;
  if (stream < 0) return FSKHIP_OK;
  if (stream >= (int64_t)e->n_streams) return fail(FSKHIP_E_INVALID, "stream out of range");
  const size_t cap = capacity ? capacity : 1;
  HIP_TRY(hipMalloc((void **)&e->S.trace_amp, sizeof(double) * cap));
  HIP_TRY(hipMalloc((void **)&e->S.trace_post, sizeof(double) * cap * 3));      // [0, cap) post filter, [cap, 3 cap) pre-filter output per input sample
  HIP_TRY(hipMalloc((void **)&e->S.trace_bit, cap));
  HIP_TRY(hipMalloc((void **)&e->S.trace_n, 2 * sizeof(uint32_t)));
  HIP_TRY(hipMemset(e->S.trace_n, 0, 2 * sizeof(uint32_t)));
  e->S.trace_stream = (uint32_t)stream;
  e->S.trace_cap = (uint32_t)cap;
  e->trace_cap = (uint32_t)cap;
  return FSKHIP_OK;
}
// {decimated samples, input samples} the trace has counted, once the device is idle
static int trace_counts(fskhip_engine *e, const size_t *n, uint32_t cnt[2]) {
  if (!e || !n) return fail(FSKHIP_E_INVALID, "null argument");
  if (!e->S.trace_n) return fail(FSKHIP_E_INVALID, "trace not enabled");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(cnt, e->S.trace_n, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}
int fskhip_trace_read_pre(fskhip_engine *e, double *pre, size_t cap, size_t *n) {
  uint32_t cnt[2] = {0, 0};
  if (const int rc = trace_counts(e, n, cnt)) return rc;
  size_t m = cnt[1] < 2u * e->trace_cap ? cnt[1] : 2u * e->trace_cap;
  m = m < cap ? m : cap;
  if (pre && m) HIP_TRY(hipMemcpy(pre, e->S.trace_post + e->trace_cap, sizeof(double) * m, hipMemcpyDeviceToHost));
  // (every kernel records the reference's own scale: the per-sample fp32 kernel of lock-step engines, which carries the value times
  // the low-pass gain b0 / 2 and 2^60, divides where it records -- the host used to, by a predicate that could not tell which
  // kernel a call had taken: ADVICE r05)
  *n = cnt[1];
  return FSKHIP_OK;
}
int fskhip_trace_read(fskhip_engine *e, double *amp, double *post, uint8_t *bit, size_t cap, size_t *n) {
  uint32_t cnt[2] = {0, 0};
  if (const int rc = trace_counts(e, n, cnt)) return rc;
  size_t m = cnt[0] < e->trace_cap ? cnt[0] : e->trace_cap;
  if (m > cap) m = cap;
  if (amp && m) HIP_TRY(hipMemcpy(amp, e->S.trace_amp, sizeof(double) * m, hipMemcpyDeviceToHost));
  if (post && m) HIP_TRY(hipMemcpy(post, e->S.trace_post, sizeof(double) * m, hipMemcpyDeviceToHost));
  if (bit && m) HIP_TRY(hipMemcpy(bit, e->S.trace_bit, m, hipMemcpyDeviceToHost));
  *n = m;
  return FSKHIP_OK;
}
// Diagnostics: one stream's raw state words as the kernels carry them between launches (fsk_params.h: RF_* / IF_* order).
int fskhip_debug_state(fskhip_engine *e, uint32_t stream, double *real_out, uint32_t real_cap, uint32_t *int_out, uint32_t int_cap,
                       uint32_t *n_real, uint32_t *n_int) {
  if (!e || stream >= e->n_streams) return fail(FSKHIP_E_INVALID, "fskhip_debug_state: bad engine / stream");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t n = e->n_streams;
  for (uint32_t f = 0; f < (uint32_t)RF_COUNT && real_out && f < real_cap; f++)
    if (const int rc = read_real(e, (int)f, stream, &real_out[f])) return rc;
  for (uint32_t f = 0; f < (uint32_t)IF_COUNT && int_out && f < int_cap; f++)
    HIP_TRY(hipMemcpy(&int_out[f], e->S.is + (size_t)f * n + stream, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (n_real) *n_real = (uint32_t)RF_COUNT;
  if (n_int) *n_int = (uint32_t)IF_COUNT;
  return FSKHIP_OK;
}
}  // extern "C"
