// fsk_api.hip -- C ABI of libfskhip.so (include/fskhip.h): configure-time parameter derivation,
// device state management and kernel launches.  No torch types, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "fsk_host.h"
#include "fsk_params.h"

namespace fsk {
hipError_t launch_demod(int precision, bool uniform_ds, bool writeback, bool append, const DemodParams &P,
                        const DemodState &S, float *samples, size_t n, size_t pitch, uint8_t *out, size_t out_pitch,
                        uint32_t *out_counts, uint32_t *eod_counts, hipStream_t stream, bool split2 = false);
bool demod_fast_applicable(int precision, bool uniform_even, const DemodParams &P, const DemodState &S,
                           const float *samples, size_t pitch);
// fsk_pipe.hip: free-running front / ZIR-corrected back kernels
hipError_t launch_demod_pipe(bool writeback, bool append, const DemodParams &P, const DemodState &S, float *samples, size_t n,
                             size_t pitch, uint8_t *out, size_t out_pitch, uint32_t *out_counts,
                             uint32_t *eod_counts, hipStream_t stream);
hipError_t launch_demod_fused(bool writeback, bool append, const DemodParams &P, const DemodState &S, float *samples, size_t n,
                              size_t pitch, uint8_t *out, size_t out_pitch, uint32_t *out_counts,
                              uint32_t *eod_counts, hipStream_t stream);
hipError_t launch_demod_tail(bool writeback, bool append, int parity0, const DemodParams &P, const DemodState &S,
                             float *samples, size_t n, size_t pitch, uint8_t *out, size_t out_pitch, uint32_t *out_counts,
                             uint32_t *eod_counts, hipStream_t stream);
size_t demod_split2_lds_bytes(const DemodParams &P);
hipError_t set_demod_split2_lds_limit(size_t lds_bytes);
size_t demod_pipe_lds_bytes(const DemodParams &P);
size_t demod_fused_lds_bytes(const DemodParams &P);
// fsk_blk.hip: four waves per group, block-batched back wave
size_t demod_blk_lds_bytes(const DemodParams &P);
size_t demod_blk_lds_bytes(const DemodParams &P, uint32_t y_slots);
bool demod_blk_applicable(const DemodParams &P);
hipError_t set_blk_lds_limit(const DemodParams &P);
hipError_t launch_demod_blk(bool writeback, bool append, const DemodParams &P, const DemodState &S, float *samples, size_t n,
                             size_t pitch, uint8_t *out, size_t out_pitch, uint32_t *out_counts,
                             uint32_t *eod_counts, hipStream_t stream, uint32_t resident_wgs, uint32_t slice_tiles, uint32_t y_slots,
                             uint32_t lanes, uint32_t medium, bool *sliced_out);
uint32_t demod_blk_lanes(uint32_t n_streams, int device);
void demod_blk_plan(const DemodParams &P, uint32_t groups, int device, uint32_t *y_slots, uint32_t *resident_wgs);
uint32_t demod_blk_slices(const DemodParams &P, const DemodState &S, size_t n, uint32_t resident_wgs, uint32_t slice_tiles,
                          uint32_t *slice_tiles_out);
size_t demod_blk_queue_words(uint32_t groups);
// fsk_blk6.hip: seven waves per group, for batches that leave every workgroup a compute unit of its own
size_t demod_blk6_lds_bytes(const DemodParams &P, uint32_t y_slots);
uint32_t demod_blk6_y_slots(const DemodParams &P);
uint32_t demod_blk6_min_y_slots();
bool demod_blk6_applicable(const DemodParams &P);
size_t demod_blk6_max_samples();
hipError_t set_blk6_lds_limit(const DemodParams &P);
uint32_t demod_blk6_default_rolemap(uint32_t lanes, bool uniform);
hipError_t launch_demod_blk6(bool writeback, bool append, const DemodParams &P, const DemodState &S, float *samples, size_t n,
                              size_t pitch, uint8_t *out, size_t out_pitch, uint32_t *out_counts, uint32_t *eod_counts,
                              hipStream_t stream, uint32_t lanes, uint32_t y_slots, uint32_t rolemap);
hipError_t set_pipe_lds_limit(size_t pipe_bytes);
hipError_t set_demod_lds_limit(size_t lds_bytes);
size_t demod_lds_bytes(const DemodParams &P);
hipError_t launch_modulate(const ModParams &M, const double *coef, const uint8_t *payloads, const uint32_t *lens,
                           size_t payload_pitch, float *out, size_t out_pitch, uint32_t *out_lens, hipStream_t st);
hipError_t launch_synth(const ModParams &M, const double *coef, float *out, size_t n, size_t pitch,
                        uint32_t payload_len, uint64_t seed, uint32_t lead_max, double amp_lo, double amp_hi,
                        hipStream_t st);
hipError_t launch_awgn(float *buf, size_t n, size_t pitch, uint32_t n_streams, double snr_db, uint64_t seed,
                       double *sigma, hipStream_t st);
hipError_t launch_probe_read(const float *buf, size_t n, size_t pitch, uint32_t n_streams, float *sink, hipStream_t st);
uint8_t host_synth_payload_byte(uint64_t seed, uint32_t stream, uint32_t frame, uint32_t i);
// fsk_remap.hip: the state gather of fskhip_remap_streams
hipError_t launch_remap(int precision, const RemapArgs &A, const int64_t *d_map, const DemodState &D, const DemodState &S,
                        hipStream_t st);
void host_synth_stream_params(uint64_t seed, uint32_t stream, uint32_t lead_max, double amp_lo, double amp_hi,
                              uint32_t *lead, double *amp);
}  // namespace fsk

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

// ---- small device kernels for state management --------------------------------------------------
namespace {

struct StatusRaw {
  double agc_gain, sil_thr;
  uint32_t started, gsc, ring_len, sync_det, eod_total, ds_cnt;
};

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

// configure(): fresh FSKCore state for every stream (fsk.ts:101-131, 175-188; AGC gain 1.0 fsk.ts:46;
// silence.threshold 0.01 fsk.ts:128).  `matched` starts at its value for an all-zero bit history.
template <typename Real>
__global__ void init_kernel(DemodState S, uint32_t n, uint32_t matched_zero) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  Real *rs = (Real *)S.rs;
  for (int f = 0; f < RF_COUNT; f++) rs[(size_t)f * n + s] = (Real)0;
  for (int f = 0; f < IF_COUNT; f++) S.is[(size_t)f * n + s] = 0u;
  rs[(size_t)RF_agc_gain * n + s] = (Real)1.0;
  rs[(size_t)RF_nco_c * n + s] = (Real)1.0;       // (the fp64 NCO's phasor at phase 0)
  rs[(size_t)RF_sil_thr * n + s] = (Real)0.01;
  S.is[(size_t)IF_matched * n + s] = matched_zero;
  S.is[(size_t)IF_bit_wait * n + s] = kBigWait;
  S.is[(size_t)IF_zr_dph * n + s] = kHandPairs;
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

}  // namespace

// ---- engine -------------------------------------------------------------------------------------
struct fskhip_engine {
  int device = 0;
  int precision = 0;
  uint32_t n_streams = 0;
  fskhip_config cfg0{};
  std::vector<fskhip_config> cfgs;   // as given to fskhip_create: one (shared) or one per stream
  uint32_t matched_zero = 0;         // `matched` of a stream with an all-zero bit history (init_kernel)
  DemodParams P{};
  ModParams M{};
  DemodState S{};
  size_t lds_bytes = 0;
  uint32_t n_blocks = 0;
  // modulator geometry (doubles as in the reference)
  double spb = 0, bpb = 0;
  // host-side debug counters (fsk.ts:131): engine-wide totals minus per-stream baselines
  uint64_t calls = 0, total_samples = 0;
  std::vector<uint64_t> base_calls, base_samples;
  bool ds_uniform = true;
  uint32_t ds_parity = 0;        // downsample.counter shared by all streams while ds_uniform
  // what fskhip_set_option() can change (tests and measurements; none changes a result)
  bool force_generic = false;    // "force_generic": never a whole-tile kernel
  bool use_split = false;        // two waves per 64-stream group (demod_pipe_kernel): batches of fewer than two waves per SIMD
  uint32_t split_cus = 256;
  bool split_forced = false;     // "kernel" pinned one: skip the residency checks too
  bool use_blk = true;           // four waves per group with the block-batched back wave (demod_blk_kernel, fsk_blk.hip): the default
                                 // wherever it applies (dsSPB a multiple of 4, >= 8)
  uint32_t blk_resident = 0;     // workgroups of demod_blk_kernel the device holds at once; larger batches run it persistent, in time slices
  uint32_t blk_min_tiles = 0;    // calls with fewer whole tiles than this stay with round 2's kernels
  uint32_t blk_y_slots = 6;      // half tiles in the block kernel's y ring: as deep as the LDS allows at this batch size
  bool blk_y_pinned = false;     // "blk_y_slots" was set: "blk_lanes" leaves it alone
  // the exact path (fp64, fsk_demod.hip) on two waves per 64-stream group -- loads + AGC + pre-filter | the rest (SPLIT2): 0 never
  // (the default: measured SLOWER, 156 against 180 Gsamples/s at config #3 -- at two waves per SIMD the back wave has 256 registers and
  // spills 864 bytes per lane, where the one-wave kernel spreads into the accumulation registers), 1 wherever it applies
  // ("exact_waves" = 2: bit-identical, tests/test_gpu_parity.py), 2 batches of at most one group per SIMD
  uint32_t exact_split = 0;
  // "blk_resets": which of fsk_blk.hip's two kernels a call launches -- demod_blk_kernel_r, whose block path takes 'eod' resets
  // itself, pays where resets are frequent (an idle receiver bank: +50 %) and costs ~4 % where they are rare.  auto: by the
  // share of tiles the PREVIOUS call's back waves took off their fast loop (the kernels count; the totals come back with an
  // asynchronous 8-byte copy behind every launch and are looked at, without waiting, before the next one).
  uint32_t blk_medium = 3;       // 0 never, 1 always, 2 (tests) always + redo every such block sample by sample, 3 auto
  bool blk_med_now = false;      // auto's current choice
  volatile unsigned long long *h_stat = nullptr;   // pinned: {tiles, tiles off the fast loop}, {hand-off fault word, -} as the last completed copy left them
  uint32_t handoff_fault = 0;                       // sticky: a kernel's hand-off wait ran into its bound (csrc/fsk_wait.h)
  uint32_t stat_tiles = 0, stat_rare = 0;          // ... as of the last look
  uint32_t stat_skip = 0;                          // short calls since the last fetch
  // seven waves per group (demod_blk6_kernel, fsk_blk6.hip): the whole-tile kernel of batches small enough to give every workgroup a
  // compute unit of its own (uniform configurations, calls of at least six_min_tiles tiles): 0 never, 1 wherever it applies
  // ("kernel" = seven-wave), 2 auto
  uint32_t use_six = 2;
  uint32_t six_min_tiles = 8;    // shorter calls stay on the four-wave kernel (one 128-sample quantum is already 1.13 x faster on seven waves, profiles/r05_lag.txt)
  uint32_t six_y_slots = 0;      // 0 = as deep as the LDS allows
  uint32_t six_rolemap = 0;      // 0 = the default placement of the seven parts on a workgroup's waves
  int cus = 0;
  bool demodulated = false;      // a demodulate call has been issued or replayed (fskhip_set_option refuses from then on)
  uint32_t blk_lanes = 64;       // streams per workgroup of demod_blk_kernel: 64, or 32 / 16 / 8 for batches that leave CUs idle (fsk_blk.hip)
  uint32_t blk_slice_tiles = 0;  // tiles per time slice (0 = the kernel file's default, 0xFFFFFFFF = never slice)
  size_t host_slab = (size_t)-1; // samples per time slab of fskhip_demodulate_host's pipeline ((size_t)-1 = ~96 MB, 0 = no pipeline)
  bool last_sliced = false;
  uint64_t pushes = 0;           // decimated samples since create (lock-step engines): the amplitude ring's write position
  bool gen_odd = false;          // fp32: the last generic-kernel launch left a decimator pair open (its partial sums are in
                                 // the reference's frame, the whole-tile kernels' in the free-running one)
  const char *last_kernel = "";  // what the last fskhip_demodulate_device call launched for its whole tiles
  bool demod_ok = true;          // false: configuration the demodulator kernels do not implement
  std::string demod_why;
  uint32_t trace_cap = 0;
  // scratch for the _host entry points
  hipStream_t stream = nullptr;
  float *d_samples = nullptr; size_t d_samples_cap = 0;
  float *d_samples2 = nullptr; size_t d_samples2_cap = 0;   // second time slab of fskhip_demodulate_host's pipeline
  hipStream_t copy_stream = nullptr;                        // its H2D stream
  hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_used_up[2] = {nullptr, nullptr};
  uint8_t *d_out = nullptr; size_t d_out_cap = 0;
  uint32_t *d_counts = nullptr, *d_eod = nullptr, *d_lens = nullptr;
  uint8_t *d_payloads = nullptr; size_t d_payloads_cap = 0;
  StatusRaw *d_status = nullptr;
  double *d_sigma = nullptr;
  unsigned long long *d_clock = nullptr;   // fskhip_clock_probe_*: {shader cycles, 100 MHz ticks}
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  hipStream_t timing_stream = nullptr;
};

int fsk::engine_device(const fskhip_engine *e) { return e->device; }
namespace fsk {
const ModParams &engine_mod_params(const fskhip_engine *e) { return e->M; }
const double *engine_coef(const fskhip_engine *e) { return e->S.coef; }
// upper bound on the bytes one call can return per stream: a byte takes bitsPerByte (>= 8) bit times of spb samples
size_t engine_max_bytes(const fskhip_engine *e, size_t n_per_stream) {
  const size_t spb = e->M.spb ? e->M.spb : 1;
  return n_per_stream / (4 * spb) + 8;
}
// everything fskhip_demodulate_device's choice of launches depends on besides its arguments
uint32_t engine_launch_key(const fskhip_engine *e) {
  return (e->ds_uniform ? 1u : 0u) | (e->ds_parity << 1) | (e->force_generic ? 4u : 0u) | (e->timing ? 8u : 0u) |
         (e->use_split ? 32u : 0u) | (e->gen_odd ? 64u : 0u) | (e->P.quality ? 256u : 0u) |
         (e->S.trace_stream != 0xFFFFFFFFu ? 16u : 0u) | (e->use_blk ? 512u : 0u) | ((uint32_t)(e->pushes & 3u) << 10) |
         ((e->blk_medium == 3u ? e->blk_med_now : e->blk_medium != 0u) ? 4096u : 0u) | (e->use_six << 13);
}
// "blk_resets" = auto: tiles, and tiles the block path with resets took or would be given, of a sample of the groups since the
// last look (whatever the last completed copy brought; nothing new = the choice stands).  It wins from about one tile in six on.
void engine_refresh_kernel_choice(fskhip_engine *e) {
  if (e->blk_medium != 3u || !e->h_stat) return;
  const unsigned long long hs = *e->h_stat;
  const uint32_t tiles = (uint32_t)hs, rare = (uint32_t)(hs >> 32);
  const uint32_t dt = tiles - e->stat_tiles, dr = rare - e->stat_rare;
  if (dt == 0u) return;
  // (with hysteresis: the two kernels count slightly different things -- the plain one cannot tell whether a tile it sends
  // down its per-sample path because of a lane's own span also holds a sync candidate)
  e->blk_med_now = (double)dr >= (e->blk_med_now ? 0.10 : 0.20) * (double)dt;
  e->stat_tiles = tiles; e->stat_rare = rare;
}
// ... and the copy that brings the totals back, behind a launch of the four- or seven-wave kernel: behind every long call, behind
// every eighth of a run of short ones (the copy is ~3 us of the stream's time, 7 % of a 128-sample call of 65 536 streams)
static hipError_t engine_fetch_blk_stat(fskhip_engine *e, size_t n_fast, hipStream_t st) {
  if (e->blk_medium != 3u || !e->h_stat || !e->S.blk_stat) return hipSuccess;
  bool fetch = n_fast >= 4096 || (++e->stat_skip & 7u) == 0u;
  if (!fetch) {                                      // (a call being captured into a graph is replayed many times: it fetches)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    fetch = hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
  }
  return fetch ? hipMemcpyAsync((void *)e->h_stat, e->S.blk_stat, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) : hipSuccess;
}
void engine_note_replayed_call(fskhip_engine *e, size_t n) {
  e->demodulated = true;
  e->calls += 1;
  e->total_samples += n;
  e->pushes += (e->ds_parity + n) >> 1;     // (the amplitude ring's position moves with a replayed call too)
  e->ds_parity = (e->ds_parity + (uint32_t)(n & 1)) & 1u;
}
}  // namespace fsk

static void ref_butter_lp(double cutoff, double sr, double b[3], double a[3]) {  // filters.ts:180-192
  double nyquist = sr / 2;
  double nc = cutoff / nyquist;
  double c = std::tan(M_PI * nc / 2);
  double c2 = c * c;
  double s2c = M_SQRT2 * c;
  double den = 1 + s2c + c2;
  b[0] = c2 / den; b[1] = 2 * c2 / den; b[2] = c2 / den;
  a[0] = 1; a[1] = (2 * c2 - 2) / den; a[2] = (1 - s2c + c2) / den;
}
static void ref_butter_hp(double cutoff, double sr, double b[3], double a[3]) {  // filters.ts:200-212
  double nyquist = sr / 2;
  double nc = cutoff / nyquist;
  double c = std::tan(M_PI * nc / 2);
  double c2 = c * c;
  double s2c = M_SQRT2 * c;
  double den = 1 + s2c + c2;
  b[0] = 1 / den; b[1] = -2 / den; b[2] = 1 / den;
  a[0] = 1; a[1] = (2 * c2 - 2) / den; a[2] = (1 - s2c + c2) / den;
}
static void ref_butter_bp(double fc, double bwHz, double sr, double b[3], double a[3]) {  // filters.ts:221-234
  double omega = 2 * M_PI * fc / sr;
  double bw = 2 * M_PI * bwHz / sr;
  double c = std::tan(bw / 2);
  double d = 2 * std::cos(omega);
  double c2 = c * c;
  double den = 1 + c + c2;
  b[0] = c / den; b[1] = 0; b[2] = -c / den;
  a[0] = 1; a[1] = (-d * (1 + c2)) / den; a[2] = (1 - c + c2) / den;
}

template <typename T>
static int ensure(T *&p, size_t &cap, size_t need) {
  if (need <= cap) return FSKHIP_OK;
  if (p) (void)hipFree(p);
  p = nullptr; cap = 0;
  hipError_t err = hipMalloc((void **)&p, need * sizeof(T));
  if (err != hipSuccess) return fail(FSKHIP_E_NOMEM, "hipMalloc(%zu): %s", need * sizeof(T), hipGetErrorString(err));
  cap = need;
  return FSKHIP_OK;
}

extern "C" {

void fskhip_butterworth_lowpass(double cutoff, double sr, double b[3], double a[3]) { ref_butter_lp(cutoff, sr, b, a); }
void fskhip_butterworth_highpass(double cutoff, double sr, double b[3], double a[3]) { ref_butter_hp(cutoff, sr, b, a); }
void fskhip_butterworth_bandpass(double fc, double bw, double sr, double b[3], double a[3]) { ref_butter_bp(fc, bw, sr, b, a); }

const char *fskhip_last_error(void) { return g_err.c_str(); }
int fskhip_abi_version(void) { return FSKHIP_ABI_VERSION; }
int fskhip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void fskhip_default_config(fskhip_config *c) {  // fsk.ts:19-33
  std::memset(c, 0, sizeof(*c));
  c->sampleRate = 48000; c->baudRate = 1200; c->markFrequency = 1650; c->spaceFrequency = 1850;
  c->preamblePattern[0] = 0x55; c->preamblePattern[1] = 0x55; c->preambleLen = 2;
  c->sfdPattern[0] = 0x7E; c->sfdLen = 1;
  c->startBits = 1; c->stopBits = 1; c->parity = 0;
  c->syncThreshold = 0.85; c->agcEnabled = 1; c->preFilterBandwidth = 800; c->adaptiveThreshold = 1;
}

static bool shared_fields_equal(const fskhip_config &a, const fskhip_config &b) {
  if (a.sampleRate != b.sampleRate || a.baudRate != b.baudRate) return false;
  if (a.preambleLen != b.preambleLen || a.sfdLen != b.sfdLen) return false;
  if (std::memcmp(a.preamblePattern, b.preamblePattern, sizeof(int32_t) * a.preambleLen)) return false;
  if (std::memcmp(a.sfdPattern, b.sfdPattern, sizeof(int32_t) * a.sfdLen)) return false;
  if (a.startBits != b.startBits || a.stopBits != b.stopBits || a.parity != b.parity) return false;
  if (a.syncThreshold != b.syncThreshold || (a.agcEnabled != 0) != (b.agcEnabled != 0)) return false;
  return true;
}

int fskhip_destroy(fskhip_engine *e) {
  if (!e) return FSKHIP_OK;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  void *bufs[] = {e->S.rs, e->S.is, e->S.poly, e->S.amp_ring, (void *)e->S.coef, (void *)e->S.nco_inc, e->d_samples,
                  e->d_samples2, e->d_out, e->d_counts, e->d_eod, e->d_lens, e->d_payloads, e->d_status, e->d_sigma,
                  e->S.trace_amp, e->S.trace_post, e->S.trace_bit, e->S.trace_n, e->S.poly_u, e->S.cu_ctr, e->S.blk_q, e->S.blk_stash, e->S.blk_stat, e->d_clock};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  if (e->h_stat) (void)hipHostFree((void *)e->h_stat);
  for (auto ev : e->ev) (void)hipEventDestroy(ev);
  for (int i = 0; i < 2; i++) {
    if (e->ev_copied[i]) (void)hipEventDestroy(e->ev_copied[i]);
    if (e->ev_used_up[i]) (void)hipEventDestroy(e->ev_used_up[i]);
  }
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return FSKHIP_OK;
}

int fskhip_create(const fskhip_config *cfgs, uint32_t n_cfgs, uint32_t n_streams, int device, int precision,
                  fskhip_engine **out) {
  if (!cfgs || !out || n_streams == 0) return fail(FSKHIP_E_INVALID, "fskhip_create: null/zero argument");
  if (n_cfgs != 1 && n_cfgs != n_streams) return fail(FSKHIP_E_INVALID, "n_cfgs must be 1 or n_streams");
  if (precision != FSKHIP_PRECISION_F32 && precision != FSKHIP_PRECISION_F64)
    return fail(FSKHIP_E_INVALID, "unknown precision %d", precision);
  const fskhip_config &c0 = cfgs[0];
  if (c0.preambleLen < 0 || c0.preambleLen > FSKHIP_MAX_PATTERN_BYTES || c0.sfdLen < 0 ||
      c0.sfdLen > FSKHIP_MAX_PATTERN_BYTES || c0.startBits < 0 || c0.stopBits < 0 || c0.startBits > 8 ||
      c0.stopBits > 8 || c0.parity < 0 || c0.parity > 2)
    return fail(FSKHIP_E_INVALID, "bad framing fields");
  if (!(c0.sampleRate > 0) || !(c0.baudRate > 0)) return fail(FSKHIP_E_INVALID, "sampleRate/baudRate must be > 0");
  for (uint32_t i = 1; i < n_cfgs; i++)
    if (!shared_fields_equal(c0, cfgs[i]))
      return fail(FSKHIP_E_UNSUPPORTED, "per-stream configs may differ only in mark/space/preFilterBandwidth (stream %u)", i);

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FSKHIP_E_NO_DEVICE, "no HIP device available (the engine has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(FSKHIP_E_NO_DEVICE, "device %d out of range (%d devices)", device, ndev);
  if (hipSetDevice(device) != hipSuccess) return fail(FSKHIP_E_NO_DEVICE, "hipSetDevice(%d) failed", device);

  fskhip_engine *e = new (std::nothrow) fskhip_engine();
  if (!e) return fail(FSKHIP_E_NOMEM, "out of host memory");
  e->device = device; e->precision = precision; e->n_streams = n_streams; e->cfg0 = c0;
  e->cfgs.assign(cfgs, cfgs + n_cfgs);
  {
    // below two waves per SIMD the one-wave-per-group kernel cannot hide its own dependency stalls; the two-wave kernel
    // gives every group two instruction streams, as long as all its workgroups' LDS tiles fit on the CUs at once.
    // (Round 2's choice; since round 3 the four-wave kernel takes every call it applies to.)
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const uint32_t n_blocks = (n_streams + 63) / 64;
    e->use_split = n_blocks < (uint32_t)cus * 8u;  // < 2 waves per SIMD (4 SIMDs per CU)
    e->split_cus = (uint32_t)cus;
  }

  // calculateParameters (fsk.ts:426-444), in doubles like the reference
  const double downsampleRate = c0.sampleRate / 2;
  e->spb = std::floor(c0.sampleRate / c0.baudRate);
  e->bpb = 8 + c0.startBits + c0.stopBits + (c0.parity != 0 ? 1 : 0);
  const double dsSPB = std::floor(downsampleRate / c0.baudRate);
  if (dsSPB < 1) { delete e; return fail(FSKHIP_E_UNSUPPORTED, "downsampledSamplesPerBit < 1"); }

  // preambleSfdBits via addByteToPattern (fsk.ts:159-173)
  std::vector<int> pat;
  auto add_byte = [&](int byte) {
    for (int i = 0; i < c0.startBits; i++) pat.push_back(0);
    for (int i = 7; i >= 0; i--) pat.push_back((byte >> i) & 1);
    if (c0.parity != 0) {
      int par = 0;
      for (int i = 0; i < 8; i++) par ^= (byte >> i) & 1;
      pat.push_back(c0.parity == 1 ? par : 1 - par);
    }
    for (int i = 0; i < c0.stopBits; i++) pat.push_back(1);
  };
  for (int i = 0; i < c0.preambleLen; i++) add_byte(c0.preamblePattern[i]);
  for (int i = 0; i < c0.sfdLen; i++) add_byte(c0.sfdPattern[i]);
  const uint32_t n_bits = (uint32_t)pat.size();
  char why[256];
  if (n_bits > 63) {
    snprintf(why, sizeof(why), "%u preamble+SFD pattern bits (max 63)", n_bits);
    e->demod_ok = false; e->demod_why = why;
  }
  const double ring_cap = ((double)n_bits + 32) * dsSPB * 1.1;  // fsk.ts:145,149
  bool frac = false;
  if (e->demod_ok && ring_cap > 4.0e9) {
    snprintf(why, sizeof(why), "sync ring capacity %.17g too large", ring_cap);
    e->demod_ok = false; e->demod_why = why;
  }
  if (e->demod_ok && ring_cap != std::floor(ring_cap)) {
    // Fractional capacity: the reference's RingBuffer freezes after floor(cap) pushes (see
    // fsk_demod.hip).  That model holds while the index sequence w -> (w+1) % cap stays
    // non-integral: w = p - n*cap exactly (all values sit on cap's ulp grid), so it turns integral
    // again after n = 2^k/gcd(m,2^k) wraps where frac(cap) = m/2^k.  Refuse if that can happen
    // within 2^40 pushes.
    frac = true;
    double f = ring_cap - std::floor(ring_cap);
    int k = 0;
    while (f != std::floor(f) && k < 80) { f *= 2; k++; }
    // f is now the odd-or-even integer m scaled by 2^k; strip common factors of two
    double m = f;
    int v2 = 0;
    while (k - v2 > 0 && std::fmod(m, 2.0) == 0.0) { m /= 2; v2++; }
    const double wraps = std::ldexp(1.0, k - v2);
    if (wraps * std::floor(ring_cap) < 1.0995e12) {
      snprintf(why, sizeof(why),
               "sync ring capacity %.17g: the reference's fractional ring index turns integral again after "
               "%.0f wraps (fsk.ts:149, utils.ts:38-48); not emulated", ring_cap, wraps);
      e->demod_ok = false; e->demod_why = why;
    }
  }
  DemodParams &P = e->P;
  P.n_streams = n_streams;
  P.d = (uint32_t)dsSPB;
  P.cadence = (uint32_t)std::floor(dsSPB / 4 + 0.5);  // Math.round
  P.n_bits = n_bits;
  P.sample_count = n_bits * P.d;
  P.frac = frac ? 1u : 0u;
  P.ring_int = e->demod_ok ? (uint32_t)std::floor(ring_cap) : 0u;
  // utils.ts:42-43: _length grows while < maxLength, so it saturates at floor(cap)+1 when fractional
  P.ring_cap = e->demod_ok ? (uint32_t)std::floor(ring_cap) + (frac ? 1u : 0u) : 0u;
  P.amp_cap = 8 * P.d;
  {
    const double total = (double)P.sample_count;
    P.matched_min = 0xFFFFFFFEu;  // never (0xFFFFFFFF is the kernels' "frame started" marker)
    if (P.sample_count > 0)
      for (uint32_t m = 0; m <= P.sample_count; m++)
        if ((double)m / total > c0.syncThreshold) { P.matched_min = m; break; }
  }
  {
    const double for_eod = e->bpb * dsSPB * 0.7;  // fsk.ts:148
    // sampleCount is >= 1 when the compare runs, so a threshold <= 1 behaves like 1
    double m = std::ceil(for_eod);
    P.eod_min = m <= 1 ? 1u : (uint32_t)m;
    // opt-in signal-quality estimates (include/fskhip.h)
    P.quality = 0;
    P.q_eod_n = (uint32_t)std::floor(for_eod);
    P.q_last_d0 = (uint32_t)((c0.sfdLen > 0 ? c0.sfdPattern[c0.sfdLen - 1] : c0.preambleLen > 0 ? c0.preamblePattern[c0.preambleLen - 1] : 1) & 1);
  }
  P.pat_q = 0; P.pat_mask = 0;
  for (uint32_t j = 1; j < n_bits && j < 64; j++) {
    P.pat_mask |= 1ull << j;
    if (pat[n_bits - j]) P.pat_q |= 1ull << j;
  }
  P.wide = (n_bits > 31 || frac) ? 1u : 0u;
  const uint32_t matched_zero = P.d * (uint32_t)__builtin_popcountll(~P.pat_q & P.pat_mask);
  e->matched_zero = matched_zero;
  P.stop_pos = c0.parity == 0 ? 9 : 10;  // fsk.ts:348
  P.parity_on = c0.parity != 0;
  P.agc_on = c0.agcEnabled != 0;
  {
    double b[3], a[3];
    ref_butter_lp(c0.baudRate, c0.sampleRate, b, a);  // fsk.ts:458-461
    P.lp_b0 = b[0]; P.lp_b1 = b[1]; P.lp_b2 = b[2]; P.lp_a1 = a[1]; P.lp_a2 = a[2];
  }
  P.agc_attack = 1.0 - std::exp(-1.0 / (c0.sampleRate * 0.001));  // fsk.ts:48-49
  P.agc_release = 1.0 - std::exp(-1.0 / (c0.sampleRate * 0.01));
  if (!P.agc_on) { P.agc_attack = 0.0; P.agc_release = 0.0; }  // fp32 kernels run the AGC block as a no-op
  P.f_lp_b0 = (float)P.lp_b0; P.f_lp_b0h = (float)(0.5 * P.lp_b0); P.f_lp_a2 = (float)P.lp_a2;
  // delta = 1 + a1 + a2 formed in f64, then rounded (see fsk_demod.hip lp32)
  P.f_lp_delta = (float)(1.0 + P.lp_a1 + P.lp_a2);
  P.f_agc_att = (float)P.agc_attack; P.f_agc_rel = (float)P.agc_release;

  ModParams &M = e->M;
  M.n_streams = n_streams;
  M.spb = (uint32_t)e->spb;
  M.bits_per_byte = (uint32_t)e->bpb;
  M.start_bits = c0.startBits; M.stop_bits = c0.stopBits; M.parity = c0.parity;
  M.exact_sin = precision == FSKHIP_PRECISION_F64 ? 1u : 0u;
  M.n_pre = c0.preambleLen + c0.sfdLen;
  for (int i = 0; i < c0.preambleLen; i++) M.pre[i] = (uint8_t)c0.preamblePattern[i];
  for (int i = 0; i < c0.sfdLen; i++) M.pre[c0.preambleLen + i] = (uint8_t)c0.sfdPattern[i];

  e->n_blocks = (n_streams + 63) / 64;
  e->lds_bytes = demod_lds_bytes(P);
  if (e->demod_ok && e->lds_bytes > 160 * 1024) {
    snprintf(why, sizeof(why), "dsSPB %u needs %zu B of LDS per wave (> 160 KiB)", P.d, e->lds_bytes);
    e->demod_ok = false; e->demod_why = why;
  }
  // per-stream constants (fsk.ts:451-456, 228, 404)
  std::vector<double> coef((size_t)CF_COUNT * n_streams);
  std::vector<uint64_t> inc(n_streams);
  for (uint32_t s = 0; s < n_streams; s++) {
    const fskhip_config &c = cfgs[n_cfgs == 1 ? 0 : s];
    const double center = (c.markFrequency + c.spaceFrequency) / 2;
    const double span = std::fabs(c.spaceFrequency - c.markFrequency);
    const double carson = 2 * (span / 2 + c.baudRate);
    const double bw = c.preFilterBandwidth > carson ? c.preFilterBandwidth : carson;
    double b[3], a[3];
    ref_butter_bp(center, bw, c.sampleRate, b, a);
    coef[(size_t)CF_bp_b0 * n_streams + s] = b[0];
    coef[(size_t)CF_bp_a1 * n_streams + s] = a[1];
    coef[(size_t)CF_bp_a2 * n_streams + s] = a[2];
    coef[(size_t)CF_omega * n_streams + s] = 2 * M_PI * center / c.sampleRate;
    coef[(size_t)CF_mark_w * n_streams + s] = 2 * M_PI * c.markFrequency / c.sampleRate;
    coef[(size_t)CF_space_w * n_streams + s] = 2 * M_PI * c.spaceFrequency / c.sampleRate;
    for (int k = 1; k <= 3; k++) {
      const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)k * (long double)center /
                              (long double)c.sampleRate;
      coef[(size_t)(CF_w1_re + 2 * (k - 1)) * n_streams + s] = (double)cosl(ang);
      coef[(size_t)(CF_w1_im + 2 * (k - 1)) * n_streams + s] = (double)sinl(ang);
    }
    // NCO increment as a 64-bit fraction of a turn: frac(center/sr) * 2^64
    long double turns = (long double)center / (long double)c.sampleRate;
    turns -= std::floor(turns);
    long double scaled = turns * 18446744073709551616.0L;
    inc[s] = scaled >= 18446744073709551615.0L ? 0xFFFFFFFFFFFFFFFFull : (uint64_t)(scaled + 0.5L);
  }

  P.uni_cfg = n_cfgs == 1 ? 1u : 0u;
  {
    const double b0 = coef[(size_t)CF_bp_b0 * n_streams], a1 = coef[(size_t)CF_bp_a1 * n_streams],
                 a2 = coef[(size_t)CF_bp_a2 * n_streams];
    P.u_bp_b0h = (float)(b0 * (0.5 * P.lp_b0));
    P.u_bp_na1 = (float)(-a1); P.u_bp_na2 = (float)(-a2);
    P.u_bp_c1y = (float)(a1 * a1 - a2); P.u_bp_c2y = (float)(a1 * a2);
    P.u_w1_re = (float)coef[(size_t)CF_w1_re * n_streams]; P.u_w1_im = (float)coef[(size_t)CF_w1_im * n_streams];
    P.u_w2_re = (float)coef[(size_t)CF_w2_re * n_streams]; P.u_w2_im = (float)coef[(size_t)CF_w2_im * n_streams];
    const uint64_t inc2 = inc[0] << 1, inc16 = inc[0] << 4;
    P.u_inc2_lo = (uint32_t)inc2; P.u_inc2_hi = (uint32_t)(inc2 >> 32);
    P.u_inc16_lo = (uint32_t)inc16; P.u_inc16_hi = (uint32_t)(inc16 >> 32);
    P.u_inc_lo = (uint32_t)inc[0]; P.u_inc_hi = (uint32_t)(inc[0] >> 32);
  }
  {
    // fsk_pipe.hip: zero-input response of the I/Q low-pass (y[n] = -a1 y[n-1] - a2 y[n-2]) as pair sums
    // q[m] = Z[2m] + Z[2m+1]:  q[m+2] = (a1^2 - 2 a2) q[m+1] - a2^2 q[m]  (the squared poles), and the map from the next
    // two pair sums back to the filter state (Z[n-1], Z[n-1] - Z[n-2]) at an even n (tools/zir_model.py)
    const double a1 = P.lp_a1, a2 = P.lp_a2;
    P.z_c1 = (float)(a1 * a1 - 2 * a2);
    P.z_c2 = (float)(a2 * a2);
    auto q_of = [&](double z1, double z2, double &q0, double &q1) {
      double Z[6] = {z2, z1, 0, 0, 0, 0};
      for (int i = 2; i < 6; i++) Z[i] = -a1 * Z[i - 1] - a2 * Z[i - 2];
      q0 = Z[2] + Z[3]; q1 = Z[4] + Z[5];
    };
    double l00, l10, l01, l11;           // q = L (zeta1, zeta2)
    q_of(1, 0, l00, l10);
    q_of(0, 1, l01, l11);
    const double det = l00 * l11 - l01 * l10;
    const double i00 = l11 / det, i01 = -l01 / det, i10 = -l10 / det, i11 = l00 / det;   // (zeta1, zeta2) = Linv (q0, q1)
    P.z_ya = (float)i00; P.z_yb = (float)i01;
    P.z_va = (float)(i00 - i10); P.z_vb = (float)(i01 - i11);
  }

#define CREATE_TRY(expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      int rc = fail(_e == hipErrorOutOfMemory ? FSKHIP_E_NOMEM : FSKHIP_E_HIP, "%s: %s", #expr,   \
                    hipGetErrorString(_e));                                                       \
      fskhip_destroy(e);                                                                          \
      return rc;                                                                                  \
    }                                                                                             \
  } while (0)
  const size_t rsz = precision == FSKHIP_PRECISION_F64 ? sizeof(double) : sizeof(float);
  CREATE_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  CREATE_TRY(hipMalloc(&e->S.rs, rsz * RF_COUNT * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->S.is, sizeof(uint32_t) * IF_COUNT * n_streams));
  const size_t poly_bytes = (P.wide ? sizeof(uint64_t) : sizeof(uint32_t)) * 64 * (size_t)P.d * e->n_blocks;
  CREATE_TRY(hipMalloc((void **)&e->S.poly, poly_bytes));
  CREATE_TRY(hipMalloc((void **)&e->S.amp_ring, sizeof(float) * (size_t)P.amp_cap * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->S.coef, sizeof(double) * coef.size()));
  CREATE_TRY(hipMalloc((void **)&e->S.nco_inc, sizeof(uint64_t) * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->d_status, sizeof(StatusRaw)));
  CREATE_TRY(hipMalloc((void **)&e->d_counts, sizeof(uint32_t) * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->d_eod, sizeof(uint32_t) * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->d_lens, sizeof(uint32_t) * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->d_sigma, sizeof(double) * n_streams));
  CREATE_TRY(hipMemcpy((void *)e->S.coef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice));
  CREATE_TRY(hipMemcpy((void *)e->S.nco_inc, inc.data(), sizeof(uint64_t) * n_streams, hipMemcpyHostToDevice));
  CREATE_TRY(hipMemset(e->S.poly, 0, poly_bytes));
  if (P.frac) {
    CREATE_TRY(hipMalloc((void **)&e->S.poly_u, poly_bytes));
    CREATE_TRY(hipMemset(e->S.poly_u, 0, poly_bytes));
  }
  CREATE_TRY(hipMemset(e->S.amp_ring, 0, sizeof(float) * (size_t)P.amp_cap * n_streams));
  CREATE_TRY(hipMalloc((void **)&e->S.cu_ctr, sizeof(uint32_t) * 2048));
  CREATE_TRY(hipMemset(e->S.cu_ctr, 0, sizeof(uint32_t) * 2048));
  {
    dim3 g((n_streams + 255) / 256), b(256);
    if (precision == FSKHIP_PRECISION_F64) hipLaunchKernelGGL(init_kernel<double>, g, b, 0, 0, e->S, n_streams, matched_zero);
    else hipLaunchKernelGGL(init_kernel<float>, g, b, 0, 0, e->S, n_streams, matched_zero);
    CREATE_TRY(hipGetLastError());
    CREATE_TRY(hipDeviceSynchronize());
  }
  if (e->demod_ok && e->lds_bytes > 48 * 1024) CREATE_TRY(set_demod_lds_limit(e->lds_bytes));
  if (e->demod_ok && precision == FSKHIP_PRECISION_F64 && !P.wide && !P.frac && demod_split2_lds_bytes(P) > 48 * 1024 && demod_split2_lds_bytes(P) <= 160 * 1024)
    CREATE_TRY(set_demod_split2_lds_limit(demod_split2_lds_bytes(P)));
  if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) e->cus = 0;
  // {tiles, tiles off the fast loop, hand-off fault word, -}: the third word is every multi-wave kernel's (csrc/fsk_wait.h)
  CREATE_TRY(hipMalloc((void **)&e->S.blk_stat, 4 * sizeof(uint32_t)));
  CREATE_TRY(hipMemset(e->S.blk_stat, 0, 4 * sizeof(uint32_t)));
  e->M.stat = e->S.blk_stat;
  if (e->demod_ok && !P.wide && !P.frac && precision == FSKHIP_PRECISION_F32 && demod_pipe_lds_bytes(P) <= 160 * 1024)
    CREATE_TRY(set_pipe_lds_limit(demod_pipe_lds_bytes(P)));
  if (e->demod_ok && precision == FSKHIP_PRECISION_F32 && demod_blk_applicable(P)) {
    CREATE_TRY(set_blk_lds_limit(P));
    CREATE_TRY(hipMalloc((void **)&e->S.blk_stash, sizeof(float) * 28u * (size_t)n_streams));
    CREATE_TRY(hipHostMalloc((void **)&e->h_stat, 2 * sizeof(unsigned long long), hipHostMallocDefault));
    e->h_stat[0] = 0ull; e->h_stat[1] = 0ull;
    e->blk_lanes = demod_blk_lanes(n_streams, device);
    demod_blk_plan(P, (n_streams + e->blk_lanes - 1u) / e->blk_lanes, device, &e->blk_y_slots, &e->blk_resident);
    if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) e->cus = 0;
    if (demod_blk6_applicable(P)) CREATE_TRY(set_blk6_lds_limit(P));
    if (e->blk_resident && e->n_blocks > e->blk_resident) {
      CREATE_TRY(hipMalloc((void **)&e->S.blk_q, sizeof(uint32_t) * demod_blk_queue_words(e->n_blocks)));
    }
  }
  e->S.trace_stream = 0xFFFFFFFFu;
#undef CREATE_TRY
  e->base_calls.assign(n_streams, 0);
  e->base_samples.assign(n_streams, 0);
  *out = e;
  return FSKHIP_OK;
}

// What FSKCore.configure() on an already configured instance leaves in place (fsk.ts:133-157 rebuilds filters, rings and
// pattern and calls resetState(), 175-188): silence.threshold (fsk.ts:128, 321-326) and the debug counters (fsk.ts:131).
// A host re-configures by creating a new engine, carrying these over from the old one and destroying that.
int fskhip_carry_over(fskhip_engine *dst, const fskhip_engine *src) {
  if (!dst || !src) return fail(FSKHIP_E_INVALID, "fskhip_carry_over: null engine");
  if (dst->n_streams != src->n_streams || dst->precision != src->precision || dst->device != src->device)
    return fail(FSKHIP_E_INVALID, "fskhip_carry_over: engines differ in stream count, precision or device");
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t n = dst->n_streams, rsz = dst->precision == FSKHIP_PRECISION_F64 ? sizeof(double) : sizeof(float);
  HIP_TRY(hipMemcpy((char *)dst->S.rs + (size_t)RF_sil_thr * n * rsz, (const char *)src->S.rs + (size_t)RF_sil_thr * n * rsz,
                    n * rsz, hipMemcpyDeviceToDevice));
  const int rows[] = {IF_sync_det, IF_eod_total};
  for (int f : rows)
    HIP_TRY(hipMemcpy(dst->S.is + (size_t)f * n, src->S.is + (size_t)f * n, n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
  dst->calls = src->calls;
  dst->total_samples = src->total_samples;
  dst->base_calls = src->base_calls;
  dst->base_samples = src->base_samples;
  return FSKHIP_OK;
}

static int handoff_check(fskhip_engine *e, bool blocking);

// Every fskhip_config field (fsk.ts:5-17): what stream i of a remap's destination and the source stream it continues must share.
static bool config_equal(const fskhip_config &a, const fskhip_config &b) {
  return shared_fields_equal(a, b) && a.markFrequency == b.markFrequency && a.spaceFrequency == b.spaceFrequency &&
         a.preFilterBandwidth == b.preFilterBandwidth && (a.adaptiveThreshold != 0) == (b.adaptiveThreshold != 0);
}
static const fskhip_config &stream_config(const fskhip_engine *e, size_t s) { return e->cfgs.size() == 1 ? e->cfgs[0] : e->cfgs[s]; }

// Stream i of dst continues stream map[i] of src as if that FSKCore had been moved, or (map[i] = -1) starts as a new one
// (include/fskhip.h).  Synchronous: every check first, then one gather launch (fsk_remap.hip), then the host-side counters.
int fskhip_remap_streams(fskhip_engine *dst, const fskhip_engine *src, const int64_t *map, uint32_t n_map) {
  if (n_map > 0 && !map) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: null map");
  for (uint32_t i = 0; i < n_map; i++)
    if (map[i] < -1) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: map[%u] = %lld (a source stream or -1)", i, (long long)map[i]);
  if (!dst || !src) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: null engine");
  if (dst == src) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: dst is src (remap into a new engine)");
  if (n_map != dst->n_streams) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: n_map %u != the destination's %u streams", n_map, dst->n_streams);
  if (dst->precision != src->precision) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: engines differ in precision (%d, %d)", dst->precision, src->precision);
  if (dst->device != src->device) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: engines are on devices %d and %d", dst->device, src->device);
  if (dst->demodulated) return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: the destination has demodulated already (remap into a fresh engine)");
  // One geometry for both engines, whatever the map (an all -1 map included): the gather reads src's state with dst's layout,
  // and dst takes over src's decimator phase and ring grid.  Every field but the per-stream tone pair / pre-filter bandwidth.
  if (!shared_fields_equal(dst->cfg0, src->cfg0) || dst->P.d != src->P.d || dst->P.amp_cap != src->P.amp_cap || dst->P.wide != src->P.wide ||
      dst->P.frac != src->P.frac || dst->P.n_bits != src->P.n_bits || dst->P.ring_cap != src->P.ring_cap)
    return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: the engines' configurations differ beyond mark/space/preFilterBandwidth "
                "(sampleRate, baudRate, framing, patterns, syncThreshold, agcEnabled must be equal)");
  uint32_t n_fresh = 0;
  int64_t frame_row = -1;   // a continued stream's source row: its free-running I/Q frame is the one dst's continued streams share
  for (uint32_t i = 0; i < n_map; i++) {
    if (map[i] < 0) { n_fresh++; continue; }
    if (map[i] >= (int64_t)src->n_streams)
      return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: map[%u] = %lld, the source has %u streams", i, (long long)map[i], src->n_streams);
    if (!config_equal(stream_config(dst, i), stream_config(src, (size_t)map[i])))
      return fail(FSKHIP_E_INVALID, "fskhip_remap_streams: the config of stream %u differs from that of source stream %lld", i, (long long)map[i]);
    if (frame_row < 0) frame_row = map[i];
  }
  HIP_TRY(hipSetDevice(dst->device));
  HIP_TRY(hipDeviceSynchronize());
  {   // a source that has reported (or now holds) a hand-off fault: its streams stopped mid-call.  Read only: src is not written.
    uint32_t w = src->handoff_fault;
    if (w == 0u && src->S.blk_stat) HIP_TRY(hipMemcpy(&w, src->S.blk_stat + 2, sizeof(w), hipMemcpyDeviceToHost));
    if (w != 0u)
      return fail(FSKHIP_E_HANDOFF, "fskhip_remap_streams: the source's multi-wave kernel ran into its hand-off bound (fault word %u): its streams cannot be continued", w);
  }

  // Lock step (one decimator phase, one ring grid for every stream) is what the whole-tile kernels need.  A continued stream
  // brings it along; a new one joins the grid -- unless the source streams are mid decimator-pair (a new one is not), the ring
  // capacity is fractional, or the source has left lock step already: then new streams start at the create-time positions and
  // the destination runs out of lock step, as after fskhip_reset of one stream mid-pair.
  bool uniform = src->ds_uniform;
  uint32_t parity = src->ds_parity;
  bool gen_odd = src->gen_odd;
  if (n_fresh == n_map) { parity = 0; gen_odd = false; }                 // only new streams: every decimator starts afresh
  else if (n_fresh > 0 && (parity != 0 || src->P.frac)) uniform = false;
  RemapArgs A{};
  A.n_dst = dst->n_streams; A.n_src = src->n_streams;
  A.d = dst->P.d; A.amp_cap = dst->P.amp_cap; A.wide = dst->P.wide; A.frac = dst->P.frac;
  A.matched_zero = dst->matched_zero;
  A.grid_src = (uniform && !src->P.frac) ? 1u : 0u;
  // (fp32, one shared configuration in dst: new streams join the frame of a CONTINUED stream -- its config is dst's, unlike that of
  // an arbitrary source row of a per-stream source, whose NCO increment and therefore frame phase may be another)
  A.frame_src = (dst->precision == FSKHIP_PRECISION_F32 && dst->P.uni_cfg && frame_row >= 0) ? 1u : 0u;
  A.frame_row = frame_row >= 0 ? (uint32_t)frame_row : 0u;
  int64_t *d_map = nullptr;
  HIP_TRY(hipMalloc((void **)&d_map, sizeof(int64_t) * n_map));
  hipError_t err = hipMemcpy(d_map, map, sizeof(int64_t) * n_map, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = launch_remap(dst->precision, A, d_map, dst->S, src->S, nullptr);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  (void)hipFree(d_map);
  if (err != hipSuccess) return fail(FSKHIP_E_HIP, "fskhip_remap_streams: %s", hipGetErrorString(err));

  // host side: the engine's clocks and, per stream, the baselines its status counters are taken against (fsk.ts:131)
  dst->calls = src->calls;
  dst->total_samples = src->total_samples;
  for (uint32_t i = 0; i < n_map; i++) {
    dst->base_calls[i] = map[i] >= 0 ? src->base_calls[(size_t)map[i]] : src->calls;
    dst->base_samples[i] = map[i] >= 0 ? src->base_samples[(size_t)map[i]] : src->total_samples;
  }
  dst->pushes = src->pushes;
  dst->ds_parity = parity;
  dst->ds_uniform = uniform;
  dst->gen_odd = gen_odd;
  dst->P.quality = src->P.quality;   // the signal-quality estimates belong to the streams: they go on accumulating where they did
  return FSKHIP_OK;
}

// Tuning and test switches (include/fskhip.h).  Everything here only chooses among kernels / launch shapes that compute the
// same bytes; the library itself reads no environment variable (the switches used to be
// unvalidated getenv() calls inside fskhip_create).
int fskhip_set_option(fskhip_engine *e, const char *name, const char *value) {
  if (!e || !name || !value) return fail(FSKHIP_E_INVALID, "fskhip_set_option: null argument");
  // (a flag of this engine's own calls -- not the call counters, which fskhip_carry_over copies from the old engine: ADVICE r04)
  if (e->demodulated) return fail(FSKHIP_E_INVALID, "fskhip_set_option(%s): the engine has demodulated already (set options after fskhip_create / fskhip_carry_over, before the first demodulate call)", name);
  const std::string k(name), v(value);
  auto number = [&](uint64_t lo, uint64_t hi, uint64_t *out) -> int {
    if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 12)
      return fail(FSKHIP_E_INVALID, "fskhip_set_option(%s): '%s' is not a number", name, value);
    const uint64_t x = strtoull(v.c_str(), nullptr, 10);
    if (x < lo || x > hi) return fail(FSKHIP_E_INVALID, "fskhip_set_option(%s): %s outside [%llu, %llu]", name, value, (unsigned long long)lo, (unsigned long long)hi);
    *out = x;
    return FSKHIP_OK;
  };
  uint64_t x = 0;
  int rc = FSKHIP_OK;
  if (k == "kernel") {          // which whole-tile kernel fp32 lock-step calls use
    const uint32_t n_blocks = e->n_blocks;
    e->use_six = 0u;
    if (v == "auto") { e->use_blk = true; e->split_forced = false; e->use_split = n_blocks < e->split_cus * 8u; e->use_six = 2u; }
    else if (v == "auto-r04") { e->use_blk = true; e->split_forced = false; e->use_split = n_blocks < e->split_cus * 8u; }   // (round 4's choice: never seven waves)
    else if (v == "auto-r02") { e->use_blk = false; e->split_forced = false; e->use_split = n_blocks < e->split_cus * 8u; }
    else if (v == "seven-wave" || v == "six-wave") { e->use_blk = true; e->use_split = true; e->split_forced = true; e->use_six = 1u; }   // (four waves where seven do not apply; "six-wave": its first name)
    else if (v == "four-wave") { e->use_blk = true; e->use_split = true; e->split_forced = true; }
    else if (v == "two-wave") { e->use_blk = false; e->use_split = true; e->split_forced = true; }
    else if (v == "one-wave") { e->use_blk = false; e->use_split = false; e->split_forced = true; }
    else return fail(FSKHIP_E_INVALID, "fskhip_set_option(kernel): '%s' is none of auto, auto-r04, auto-r02, seven-wave, four-wave, two-wave, one-wave", value);
    return FSKHIP_OK;
  }
  if (k == "blk_resets") {      // 1: the four-wave kernel's block path takes resets (default), 0: such blocks go sample by sample
    if (v == "auto") { e->blk_medium = 3u; return FSKHIP_OK; }
    if ((rc = number(0, 2, &x)) != FSKHIP_OK) return rc;   // (2, tests: run it, then restore the entry state and redo the block sample by sample)
    e->blk_medium = (uint32_t)x;
    return FSKHIP_OK;
  }
  if (k == "stage_min_tiles") {
    if ((rc = number(0, 1u << 30, &x)) != FSKHIP_OK) return rc;
    e->six_min_tiles = (uint32_t)x;
    return FSKHIP_OK;
  }
  if (k == "stage_y_slots") {     // (checked against what the kernel can use, as blk_y_slots is -- it used to be clamped silently)
    if (!(e->demod_ok && e->precision == FSKHIP_PRECISION_F32 && demod_blk6_applicable(e->P))) return FSKHIP_OK;   // (the seven-wave kernel does not apply: nothing to tune)
    const uint32_t lo = demod_blk6_min_y_slots(), hi = demod_blk6_y_slots(e->P);
    if ((rc = number(lo, hi, &x)) != FSKHIP_OK) return rc;
    if (x & 1u) return fail(FSKHIP_E_INVALID, "fskhip_set_option(stage_y_slots): %s is odd (whole tiles: two half tiles each)", value);
    e->six_y_slots = (uint32_t)x;
    return FSKHIP_OK;
  }
  if (k == "stage_roles") {       // measurements: the part each of the seven waves plays, e.g. 0135426 (every part exactly once)
    if (v == "auto") { e->six_rolemap = 0u; return FSKHIP_OK; }
    uint32_t m = 0, seen = 0;
    if (v.size() != 7) return fail(FSKHIP_E_INVALID, "fskhip_set_option(stage_roles): '%s' is not seven digits 0..6", value);
    for (uint32_t w = 0; w < 7; w++) {
      const uint32_t r = (uint32_t)(v[w] - '0');
      if (r > 6u || (seen & (1u << r))) return fail(FSKHIP_E_INVALID, "fskhip_set_option(stage_roles): '%s' is not a permutation of 0..6", value);
      seen |= 1u << r; m |= r << (3u * w);
    }
    e->six_rolemap = m;
    return FSKHIP_OK;
  }
  if (k == "exact_waves") {       // the fp64 kernel: auto | 1 (one wave per 64-stream group) | 2 (two: loads + AGC + pre-filter | the rest)
    if (v == "auto") { e->exact_split = 0u; return FSKHIP_OK; }     // (auto = one wave: the two-wave cut does not pay, see exact_split)
    if ((rc = number(1, 2, &x)) != FSKHIP_OK) return rc;
    e->exact_split = x == 2 ? 1u : 0u;
    return FSKHIP_OK;
  }
  if (k == "force_generic") {
    if ((rc = number(0, 1, &x)) != FSKHIP_OK) return rc;
    e->force_generic = x != 0;
    return FSKHIP_OK;
  }
  if (k == "host_slab") {
    if ((rc = number(0, 1ull << 40, &x)) != FSKHIP_OK) return rc;
    e->host_slab = (size_t)x;
    return FSKHIP_OK;
  }
  const bool blk = e->demod_ok && e->precision == FSKHIP_PRECISION_F32 && demod_blk_applicable(e->P);
  if (k == "blk_y_slots" || k == "blk_min_tiles" || k == "blk_resident" || k == "slice_tiles" || k == "blk_lanes") {
    if (!blk) return FSKHIP_OK;                       // (the four-wave kernel does not apply to this engine: nothing to tune)
    if (k == "blk_y_slots") {
      if ((rc = number(6, 28, &x)) != FSKHIP_OK) return rc;
      if (demod_blk_lds_bytes(e->P, (uint32_t)x) > 160 * 1024)
        return fail(FSKHIP_E_INVALID, "fskhip_set_option(blk_y_slots): %s slots need %zu B of LDS (> 160 KiB) at dsSPB %u", value,
                    demod_blk_lds_bytes(e->P, (uint32_t)x), e->P.d);
      e->blk_y_slots = (uint32_t)x;
      e->blk_y_pinned = true;                          // (a later "blk_lanes" re-plans the depth only if it was not asked for)
    } else if (k == "blk_lanes") {                    // streams per workgroup: auto (what the device's CU count suggests) | 64 | 32 | 16 | 8
      if (v == "auto") {
        e->blk_lanes = demod_blk_lanes(e->n_streams, e->device);
        uint32_t y = 0, res = 0;
        demod_blk_plan(e->P, (e->n_streams + e->blk_lanes - 1u) / e->blk_lanes, e->device, &y, &res);
        if (y && !e->blk_y_pinned) e->blk_y_slots = y;
        return FSKHIP_OK;
      }
      if ((rc = number(8, 64, &x)) != FSKHIP_OK) return rc;
      if (x & (x - 1u)) return fail(FSKHIP_E_INVALID, "fskhip_set_option(blk_lanes): %s is none of auto, 64, 32, 16, 8", value);
      e->blk_lanes = (uint32_t)x;
      {   // the ring depth follows the workgroup count the new width gives; a "blk_resident" pinned by a test stays
        uint32_t y = 0, res = 0;
        demod_blk_plan(e->P, (e->n_streams + e->blk_lanes - 1u) / e->blk_lanes, e->device, &y, &res);
        if (y && !e->blk_y_pinned) e->blk_y_slots = y;
      }
    } else if (k == "blk_min_tiles") {
      if ((rc = number(0, 1u << 30, &x)) != FSKHIP_OK) return rc;
      e->blk_min_tiles = (uint32_t)x;
    } else if (k == "blk_resident") {                 // tests: a "device" that holds only this many workgroups at once
      if ((rc = number(1, 1u << 20, &x)) != FSKHIP_OK) return rc;
      e->blk_resident = (uint32_t)x;
      e->blk_lanes = 64u;                             // (a device that small has no idle CUs to spread narrow groups over)
      if (e->n_blocks > e->blk_resident && !e->S.blk_q) {
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipMalloc((void **)&e->S.blk_q, sizeof(uint32_t) * demod_blk_queue_words(e->n_blocks)));
      }
    } else {
      if (v == "off") { e->blk_slice_tiles = 0xFFFFFFFFu; return FSKHIP_OK; }
      if ((rc = number(1, 1u << 24, &x)) != FSKHIP_OK) return rc;
      e->blk_slice_tiles = (uint32_t)x;
    }
    return FSKHIP_OK;
  }
  return fail(FSKHIP_E_INVALID, "fskhip_set_option: unknown option '%s'", name);
}

uint32_t fskhip_n_streams(const fskhip_engine *e) { return e ? e->n_streams : 0; }
size_t fskhip_max_bytes(const fskhip_engine *e, size_t n_per_stream) { return e ? engine_max_bytes(e, n_per_stream) : 0; }
const char *fskhip_last_kernel(const fskhip_engine *e) { return e ? e->last_kernel : ""; }
uint32_t fskhip_blk_lanes(const fskhip_engine *e) {
  return (e && e->demod_ok && e->precision == FSKHIP_PRECISION_F32 && demod_blk_applicable(e->P)) ? e->blk_lanes : 0u;
}

// append_first: this launch sequence continues a call that has produced output already (a time slab of
// fskhip_demodulate_host's pipeline); count_call: it is (the first part of) a demodulateData() call of its own
// The hand-off fault word (csrc/fsk_wait.h): a wave of a multi-wave kernel got nowhere in FSK_SPIN_CAP polls of one wait and ended
// its launch early.  Sticky: the streams of that workgroup are mid-call, the engine is to be destroyed.  `blocking`: read the word
// from the device (the caller has synchronised); otherwise whatever the last completed statistics copy brought (costs nothing).
static int handoff_check(fskhip_engine *e, bool blocking) {
  if (e->handoff_fault == 0u) {
    uint32_t w = 0;
    if (blocking) {
      if (e->S.blk_stat && hipMemcpy(&w, e->S.blk_stat + 2, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) w = 0;
    } else if (e->h_stat) {
      w = (uint32_t)e->h_stat[1];
    }
    e->handoff_fault = w;
  }
  if (e->handoff_fault != 0u)
    return fail(FSKHIP_E_HANDOFF, "a hand-off wait of a multi-wave kernel ran into its bound (fault word %u, last kernel %s): destroy the engine",
                e->handoff_fault, e->last_kernel);
  return FSKHIP_OK;
}

static int demod_device_impl(fskhip_engine *e, float *d_samples, size_t n, size_t pitch, uint8_t *d_out,
                             size_t out_pitch, uint32_t *d_out_counts, uint32_t *d_eod_counts, uint32_t flags,
                             void *hip_stream, bool append_first, bool count_call) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "FSK demodulator not configured");
  if (!d_out_counts || (n > 0 && !d_samples) || (out_pitch > 0 && !d_out))
    return fail(FSKHIP_E_INVALID, "fskhip_demodulate_device: null buffer");
  if (pitch < n) return fail(FSKHIP_E_INVALID, "pitch %zu < n_per_stream %zu", pitch, n);
  if (!e->demod_ok) return fail(FSKHIP_E_UNSUPPORTED, "demodulator unsupported for this configuration: %s", e->demod_why.c_str());
  if (const int hrc = handoff_check(e, false)) return hrc;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const bool timed = e->timing;
  if (timed) {
    if (e->ev_used + 2 > e->ev.size()) {
      hipEvent_t a, b;
      HIP_TRY(hipEventCreate(&a));
      HIP_TRY(hipEventCreate(&b));
      e->ev.push_back(a); e->ev.push_back(b);
    }
    e->timing_stream = st;
    HIP_TRY(hipEventRecord(e->ev[e->ev_used], st));
  }
  {
    const bool wb = (flags & FSKHIP_DEMOD_WRITEBACK_AGC) != 0;
    // Lock-step fp32 batches with narrow integer-capacity rings never leave fsk_pipe.hip's arithmetic: a head of
    // single samples up to an even decimator parity and a 16-byte boundary, whole 16-sample tiles, a tail of single
    // samples -- so cutting a stream into calls of any lengths changes nothing, bit for bit.  Everything else (fp64,
    // wide / fractional rings, streams out of lock step) is the generic kernel's.
    e->last_kernel = "";
    if (n > 0 && !e->force_generic && !e->gen_odd && demod_fast_applicable(e->precision, e->ds_uniform, e->P, e->S, d_samples, pitch)) {
      const size_t wgs_per_cu = (e->n_blocks + e->split_cus - 1) / e->split_cus;
      const size_t pipe_lds = demod_pipe_lds_bytes(e->P);
      const bool two_wave = e->use_split && pipe_lds <= 160 * 1024 && (wgs_per_cu * pipe_lds <= 160 * 1024 || e->split_forced);
      const uint32_t p0 = e->ds_parity;
      size_t head = 0, n_fast = 0;
      bool tiles = (pitch % 4 == 0) && (uint64_t)pitch * 4u * 64u < 0x7FFFFFF0ull && (reinterpret_cast<uintptr_t>(d_samples) & 3u) == 0;
      if (tiles) {
        // The head: single samples (demod_tail_kernel) until the /2 decimator is at a pair boundary AND the amplitude
        // ring's write position is a multiple of four -- what the block kernel's quad stores need (fsk_dev.h).  At most
        // seven samples.  The tile loads that follow are 16 bytes per lane from dword-aligned addresses: a buffer that is
        // 16-byte aligned after the head is the common case and the fastest, but nothing depends on it (VERDICT r03 #6:
        // round 3 demanded both, so one odd-length call left an aligned device buffer on the per-sample kernel until
        // the parity flipped back, and a call that left the ring off its quad grid kept the engine on round 2's
        // kernels for good).
        head = p0;                                                  // closes the open pair
        const uint64_t at = e->pushes + ((p0 + head) >> 1);       // the ring's position after it
        if (e->use_blk && demod_blk_applicable(e->P)) head += 2u * (size_t)((4u - (uint32_t)(at & 3u)) & 3u);
      }
      if (e->S.trace_stream != 0xFFFFFFFFu || e->P.quality) tiles = false;   // diagnostics (traces, quality estimates) run on the sample-granular kernel
      if (tiles && head < n) n_fast = (n - head) & ~(size_t)15;
      if (!n_fast) head = n;   // all of it sample by sample
      bool app = append_first;
      if (head) {
        HIP_TRY(launch_demod_tail(wb, app, (int)p0, e->P, e->S, d_samples, head, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, st));
        e->last_kernel = "fsk::demod_tail_kernel";
        app = true;
      }
      if (n_fast) {
        const size_t blk_lds = demod_blk_lds_bytes(e->P);
        // the block kernel stores amplitudes a quad at a time: the ring's write position at its first sample must be a
        // multiple of four (it is unless earlier calls had odd lengths: those calls then stay with the per-sample kernels)
        const bool quad_aligned = ((e->pushes + ((p0 + head) >> 1)) & 3u) == 0u;
        // Batches beyond one round of resident workgroups run the block kernel persistently, in time slices; a call too
        // short for two slices would run it in several rounds of one workgroup per group, each paying the four-wave
        // pipeline's fill and drain, and round 2's kernels are faster there (262 144 streams x 128-sample quanta, the
        // FSKProcessor loop: 0.195 against 0.247 ms; x 4 096 samples 384 against 370 Gsamples/s:
        // profiles/r03_short_calls.txt)
        const bool blk_fits = e->blk_lanes != 64u || !(e->blk_resident && e->n_blocks > e->blk_resident) ||
                              demod_blk_slices(e->P, e->S, n_fast, e->blk_resident, e->blk_slice_tiles, nullptr) >= 2u;
        if (e->use_blk && demod_blk_applicable(e->P) && blk_lds <= 160 * 1024 && (quad_aligned || e->split_forced) &&
            ((blk_fits && n_fast / 16 >= e->blk_min_tiles) || e->split_forced)) {
          engine_refresh_kernel_choice(e);
          uint32_t med = e->blk_medium == 3u ? (e->blk_med_now ? 1u : 0u) : e->blk_medium;
          // seven waves per group: every workgroup a compute unit to itself (in narrow groups -- <= 32 streams -- the stages that
          // are not recurrences spread over the idle lanes), a uniform configuration, a call long enough to fill seven stages.
          // Measured against the four-wave kernel: x 1.56 at 2 048 streams, x 1.48 at 4 096, x 1.42 at 8 192, x 1.13 with whole-wave
          // groups at 16 384 (profiles/r05_lag.txt).  Idle receiver banks included: its frame wave takes own-span tiles on the
          // block path with resets too.
          const uint32_t six_blocks = (e->n_streams + e->blk_lanes - 1u) / e->blk_lanes;
          const bool six = e->use_six != 0u && quad_aligned && demod_blk6_applicable(e->P) && n_fast <= demod_blk6_max_samples() &&
                           (e->use_six == 1u || (e->cus > 0 && six_blocks <= (uint32_t)e->cus && n_fast / 16 >= e->six_min_tiles));
          if (six) {
            HIP_TRY(launch_demod_blk6(wb, app, e->P, e->S, d_samples + head, n_fast, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, st,
                                      e->blk_lanes, e->six_y_slots ? e->six_y_slots : demod_blk6_y_slots(e->P), e->six_rolemap));
            e->last_sliced = false;
            HIP_TRY(engine_fetch_blk_stat(e, n_fast, st));
            static const char *const names6[16] = {
                "fsk::demod_blk6_kernel<false, 64>", "fsk::demod_blk6_kernel<false, 32>", "fsk::demod_blk6_kernel<false, 16>", "fsk::demod_blk6_kernel<false, 8>",
                "fsk::demod_blk6_kernel<true, 64>", "fsk::demod_blk6_kernel<true, 32>", "fsk::demod_blk6_kernel<true, 16>", "fsk::demod_blk6_kernel<true, 8>",
                // (round 6: per-stream tone pairs -- <write-back, streams per workgroup, uniform = false>)
                "fsk::demod_blk6_kernel<false, 64, false>", "fsk::demod_blk6_kernel<false, 32, false>", "fsk::demod_blk6_kernel<false, 16, false>", "fsk::demod_blk6_kernel<false, 8, false>",
                "fsk::demod_blk6_kernel<true, 64, false>", "fsk::demod_blk6_kernel<true, 32, false>", "fsk::demod_blk6_kernel<true, 16, false>", "fsk::demod_blk6_kernel<true, 8, false>"};
            e->last_kernel = names6[(e->P.uni_cfg ? 0 : 8) + (wb ? 4 : 0) + (e->blk_lanes == 64u ? 0 : e->blk_lanes == 32u ? 1 : e->blk_lanes == 16u ? 2 : 3)];
          } else {
          HIP_TRY(launch_demod_blk(wb, app, e->P, e->S, d_samples + head, n_fast, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, st,
                                   e->blk_resident, e->blk_slice_tiles, e->blk_y_slots, e->blk_lanes, med, &e->last_sliced));
          HIP_TRY(engine_fetch_blk_stat(e, n_fast, st));
          static const char *const names[12] = {
              "fsk::demod_blk_kernel<false, false, false>", "fsk::demod_blk_kernel<false, false, true>",
              "fsk::demod_blk_kernel<false, true, false>", "fsk::demod_blk_kernel<false, true, true>",
              "fsk::demod_blk_kernel<true, false, false>", "fsk::demod_blk_kernel<true, false, true>",
              "fsk::demod_blk_kernel<true, true, false>", "fsk::demod_blk_kernel<true, true, true>",
              "fsk::demod_blk_kernel_r<false, false>", "fsk::demod_blk_kernel_r<false, true>",
              "fsk::demod_blk_kernel_r<true, false>", "fsk::demod_blk_kernel_r<true, true>"};
          static const char *const names_rp[4] = {"fsk::demod_blk_kernel_rp<false, false>", "fsk::demod_blk_kernel_rp<false, true>",
                                                  "fsk::demod_blk_kernel_rp<true, false>", "fsk::demod_blk_kernel_rp<true, true>"};
          if (med && !e->P.uni_cfg) e->last_kernel = names_rp[(wb ? 2 : 0) + (e->last_sliced ? 1 : 0)];
          else e->last_kernel = med ? names[8 + (wb ? 2 : 0) + (e->last_sliced ? 1 : 0)]                  // <writeback, time-sliced>
                                    : names[(wb ? 4 : 0) + (e->P.uni_cfg ? 2 : 0) + (e->last_sliced ? 1 : 0)];   // <writeback, uniform, time-sliced>
          }
        } else if (two_wave) {
          HIP_TRY(launch_demod_pipe(wb, app, e->P, e->S, d_samples + head, n_fast, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, st));
          e->last_kernel = wb ? (e->P.uni_cfg ? "fsk::demod_pipe_kernel<true, true>" : "fsk::demod_pipe_kernel<true, false>")
                              : (e->P.uni_cfg ? "fsk::demod_pipe_kernel<false, true>" : "fsk::demod_pipe_kernel<false, false>");
        } else {
          HIP_TRY(launch_demod_fused(wb, app, e->P, e->S, d_samples + head, n_fast, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, st));
          e->last_kernel = wb ? (e->P.uni_cfg ? "fsk::demod_fused_kernel<true, true>" : "fsk::demod_fused_kernel<true, false>")
                              : (e->P.uni_cfg ? "fsk::demod_fused_kernel<false, true>" : "fsk::demod_fused_kernel<false, false>");
        }
        app = true;
        const size_t done = head + n_fast;
        if (done < n)
          HIP_TRY(launch_demod_tail(wb, true, 0, e->P, e->S, d_samples + done, n - done, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, st));
      }
    } else {
      e->P.nco_anchor = (uint32_t)(e->total_samples & 31u);   // (fp64: where the NCO phasor is re-evaluated; fsk_demod.hip, mix_lp)
      const bool split2 = e->precision == FSKHIP_PRECISION_F64 && e->ds_uniform && !e->P.wide && !e->P.frac && e->S.trace_stream == 0xFFFFFFFFu &&
                          !e->P.quality && demod_split2_lds_bytes(e->P) <= 160 * 1024 &&
                          (e->exact_split == 1u || (e->exact_split == 2u && e->cus > 0 && e->n_blocks <= 4u * (uint32_t)e->cus && n >= 64));
      HIP_TRY(launch_demod(e->precision, e->ds_uniform, wb, append_first, e->P, e->S, d_samples, n, pitch, d_out, out_pitch,
                           d_out_counts, d_eod_counts, st, split2));
      e->last_kernel = split2 ? "fsk::demod_kernel<double, ..., two waves>" : e->precision == FSKHIP_PRECISION_F64 ? "fsk::demod_kernel<double, ...>" : "fsk::demod_kernel<float, ...>";
      // the generic kernel keeps an open decimator pair's partial sums in the reference's own frame: stay with it
      // until the pair is closed
      if (n > 0) e->gen_odd = e->precision == FSKHIP_PRECISION_F32 && ((e->ds_parity + (uint32_t)(n & 1)) & 1u) != 0;
    }
  }
  if (timed) {
    HIP_TRY(hipEventRecord(e->ev[e->ev_used + 1], st));
    e->ev_used += 2;
  }
  e->demodulated = true;
  e->calls += count_call ? 1 : 0;
  e->total_samples += n;
  e->pushes += (e->ds_parity + n) >> 1;
  e->ds_parity = (e->ds_parity + (uint32_t)(n & 1)) & 1u;
  return FSKHIP_OK;
}

int fskhip_demodulate_device(fskhip_engine *e, float *d_samples, size_t n, size_t pitch, uint8_t *d_out,
                             size_t out_pitch, uint32_t *d_out_counts, uint32_t *d_eod_counts, uint32_t flags,
                             void *hip_stream) {
  return demod_device_impl(e, d_samples, n, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, flags, hip_stream, false, true);
}

// Host buffers in, bytes out.  A call longer than one time slab is a two-buffer pipeline over TIME: slab j+1 crosses PCIe
// on the copy stream while slab j is demodulated on the compute stream.  Cutting along time needs no sub-batch launches,
// and the engine gives the same bytes for any cut (the reference is a streaming state machine, fsk.ts:190-222).  The
// copies only overlap if `samples` is page-locked (fskhip_host_alloc, or any pinned buffer of the caller); with pageable
// memory the runtime stages each copy itself and the pipeline degrades gracefully to what one big copy costs.
int fskhip_demodulate_host(fskhip_engine *e, float *samples, size_t n, size_t pitch, uint8_t *out, size_t out_pitch,
                           uint32_t *out_counts, uint32_t *eod_counts, uint32_t flags) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "FSK demodulator not configured");
  if (!out_counts || (n > 0 && !samples) || (out_pitch > 0 && !out)) return fail(FSKHIP_E_INVALID, "null buffer");
  if (pitch < n) return fail(FSKHIP_E_INVALID, "pitch %zu < n_per_stream %zu", pitch, n);
  HIP_TRY(hipSetDevice(e->device));
  const size_t S = e->n_streams;
  const bool wb = (flags & FSKHIP_DEMOD_WRITEBACK_AGC) != 0;
  // slab length: ~96 MB of samples per slab, a multiple of 16 (whole tiles, even decimator parity), at least 4096
  size_t slab = ((size_t)96 << 20) / (S * sizeof(float));
  slab = slab < 4096 ? 4096 : slab;
  slab &= ~(size_t)15;
  if (e->host_slab != (size_t)-1) slab = e->host_slab & ~(size_t)15;   // fskhip_set_option("host_slab"): tests / measurements
  const bool piped = slab > 0 && n > slab + slab / 2;
  const size_t len0 = piped ? slab + slab / 2 : n;    // (the last slab of a pipelined call takes the remainder, < 1.5 slabs)
  // device copies keep a row pitch that is a multiple of 4 floats so the 16-B tile loads apply.  A stream whose /2
  // decimator is mid-pair (an earlier call had an odd length) is staged THREE floats into its row: the one sample that
  // closes the pair then also reaches the next 16-byte boundary, and the rest of the call runs on whole tiles -- staged
  // at the row start it would need an odd head for the parity and a multiple of four for the alignment, i.e. every
  // later even-length call would run sample by sample (fsk_api.hip's silent performance cliff).
  const size_t dpitch = ((len0 + 3 + 3) & ~(size_t)3) ? ((len0 + 3 + 3) & ~(size_t)3) : 4;
  auto shift = [&]() -> size_t { return (e->precision == FSKHIP_PRECISION_F32 && e->ds_uniform && (e->ds_parity & 1u)) ? 3 : 0; };
  int rc;
  if ((rc = ensure(e->d_samples, e->d_samples_cap, dpitch * S)) != FSKHIP_OK) return rc;
  if ((rc = ensure(e->d_out, e->d_out_cap, (out_pitch ? out_pitch : 1) * S)) != FSKHIP_OK) return rc;
  if (!piped) {
    float *stg = e->d_samples + shift();
    if (n > 0)
      HIP_TRY(hipMemcpy2DAsync(stg, dpitch * sizeof(float), samples, pitch * sizeof(float), n * sizeof(float), S,
                               hipMemcpyHostToDevice, e->stream));
    rc = fskhip_demodulate_device(e, stg, n, dpitch, e->d_out, out_pitch, e->d_counts, e->d_eod, flags, e->stream);
    if (rc != FSKHIP_OK) return rc;
    if (wb && n > 0)
      HIP_TRY(hipMemcpy2DAsync(samples, pitch * sizeof(float), stg, dpitch * sizeof(float), n * sizeof(float), S,
                               hipMemcpyDeviceToHost, e->stream));
  } else {
    if ((rc = ensure(e->d_samples2, e->d_samples2_cap, dpitch * S)) != FSKHIP_OK) return rc;
    if (!e->copy_stream) {
      HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
      for (int i = 0; i < 2; i++) {
        HIP_TRY(hipEventCreateWithFlags(&e->ev_copied[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_used_up[i], hipEventDisableTiming));
      }
    }
    // on a failure inside the pipeline, let what is in flight on both streams finish before the caller's buffers go away
#define PIPE_TRY(expr)                                                                               \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) {                                                                          \
      (void)hipStreamSynchronize(e->copy_stream); (void)hipStreamSynchronize(e->stream);             \
      return fail(FSKHIP_E_HIP, "%s: %s", #expr, hipGetErrorString(_e));                            \
    }                                                                                                \
  } while (0)
    float *buf[2] = {e->d_samples, e->d_samples2};
    size_t off = 0;
    for (size_t j = 0; off < n; j++) {
      // the last slab takes the remainder (up to 1.5 slabs would not be worth another round trip)
      const size_t len = (n - off > slab + slab / 2) ? slab : n - off;
      if (len + 3 > dpitch) return fail(FSKHIP_E_INVALID, "internal: slab %zu exceeds staging pitch %zu", len, dpitch);
      const int b = (int)(j & 1);
      float *stg = buf[b] + shift();               // (the parity at this slab's start: slabs are multiples of 16 samples)
      if (j >= 2) PIPE_TRY(hipStreamWaitEvent(e->copy_stream, e->ev_used_up[b], 0));   // its previous user has finished
      PIPE_TRY(hipMemcpy2DAsync(stg, dpitch * sizeof(float), samples + off, pitch * sizeof(float), len * sizeof(float), S,
                               hipMemcpyHostToDevice, e->copy_stream));
      PIPE_TRY(hipEventRecord(e->ev_copied[b], e->copy_stream));
      PIPE_TRY(hipStreamWaitEvent(e->stream, e->ev_copied[b], 0));
      rc = demod_device_impl(e, stg, len, dpitch, e->d_out, out_pitch, e->d_counts, e->d_eod, flags, e->stream,
                             /*append_first=*/j > 0, /*count_call=*/j == 0);
      if (rc != FSKHIP_OK) { (void)hipStreamSynchronize(e->copy_stream); (void)hipStreamSynchronize(e->stream); return rc; }
      if (wb)
        PIPE_TRY(hipMemcpy2DAsync(samples + off, pitch * sizeof(float), stg, dpitch * sizeof(float), len * sizeof(float), S,
                                 hipMemcpyDeviceToHost, e->stream));
      PIPE_TRY(hipEventRecord(e->ev_used_up[b], e->stream));
      off += len;
    }
#undef PIPE_TRY
  }
  if (out_pitch > 0) HIP_TRY(hipMemcpyAsync(out, e->d_out, out_pitch * S, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(out_counts, e->d_counts, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, e->stream));
  if (eod_counts) HIP_TRY(hipMemcpyAsync(eod_counts, e->d_eod, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->copy_stream) HIP_TRY(hipStreamSynchronize(e->copy_stream));
  if (const int hrc = handoff_check(e, true)) return hrc;
  for (size_t s = 0; s < S; s++)
    if (out_counts[s] > out_pitch) return fail(FSKHIP_E_OVERFLOW, "stream %zu produced %u bytes, slab holds %zu", s, out_counts[s], out_pitch);
  return FSKHIP_OK;
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
  const bool timed = e->timing;     // (fskhip_timing_begin / _end bracket modulate launches too: bench.py --workload mod)
  if (timed) {
    if (e->ev_used + 2 > e->ev.size()) {
      hipEvent_t a, b;
      HIP_TRY(hipEventCreate(&a));
      HIP_TRY(hipEventCreate(&b));
      e->ev.push_back(a); e->ev.push_back(b);
    }
    e->timing_stream = st;
    HIP_TRY(hipEventRecord(e->ev[e->ev_used], st));
  }
  HIP_TRY(launch_modulate(e->M, e->S.coef, d_payloads, d_lens, payload_pitch, d_out, out_pitch, d_out_lens, st));
  if (timed) {
    HIP_TRY(hipEventRecord(e->ev[e->ev_used + 1], st));
    e->ev_used += 2;
  }
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
  if ((rc = ensure(e->d_samples, e->d_samples_cap, (dpitch ? dpitch : 4) * S)) != FSKHIP_OK) return rc;
  if ((rc = ensure(e->d_payloads, e->d_payloads_cap, (payload_pitch ? payload_pitch : 1) * S)) != FSKHIP_OK) return rc;
  for (size_t s = 0; s < S; s++)
    if (lens[s] > payload_pitch) return fail(FSKHIP_E_INVALID, "lens[%zu] = %u exceeds payload_pitch %zu", s, lens[s], payload_pitch);
  if (payload_pitch > 0 && payloads)
    HIP_TRY(hipMemcpyAsync(e->d_payloads, payloads, payload_pitch * S, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_lens, lens, sizeof(uint32_t) * S, hipMemcpyHostToDevice, e->stream));
  rc = fskhip_modulate_device(e, e->d_payloads, e->d_lens, payload_pitch, e->d_samples, dpitch, e->d_counts, e->stream);
  if (rc != FSKHIP_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_lens, e->d_counts, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpy2DAsync(out, out_pitch * sizeof(float), e->d_samples, dpitch * sizeof(float),
                           out_pitch * sizeof(float), S, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (const int hrc = handoff_check(e, true)) return hrc;
  for (size_t s = 0; s < S; s++)
    if (out_lens[s] > out_pitch) return fail(FSKHIP_E_OVERFLOW, "stream %zu needs %u samples, slab holds %zu", s, out_lens[s], out_pitch);
  return FSKHIP_OK;
}

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
  if (e->precision == FSKHIP_PRECISION_F64) hipLaunchKernelGGL(status_kernel<double>, dim3(1), dim3(1), 0, 0, e->S, e->n_streams, stream, e->d_status);
  else hipLaunchKernelGGL(status_kernel<float>, dim3(1), dim3(1), 0, 0, e->S, e->n_streams, stream, e->d_status);
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
  const size_t n = e->n_streams, rsz = e->precision == FSKHIP_PRECISION_F64 ? sizeof(double) : sizeof(float);
  if (on) {   // the accumulators are contiguous rows at the end of both state arrays
    HIP_TRY(hipMemset((char *)e->S.rs + (size_t)RF_q_signal * n * rsz, 0, (size_t)(RF_COUNT - RF_q_signal) * n * rsz));
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
  const bool f64 = e->precision == FSKHIP_PRECISION_F64;
  double rv[RF_COUNT - RF_q_signal];
  uint32_t iv[IF_COUNT - IF_q_armed];
  for (int f = RF_q_signal; f < RF_COUNT; f++) {
    if (f64) {
      HIP_TRY(hipMemcpy(&rv[f - RF_q_signal], (const double *)e->S.rs + (size_t)f * n + stream, sizeof(double), hipMemcpyDeviceToHost));
    } else {
      float v;
      HIP_TRY(hipMemcpy(&v, (const float *)e->S.rs + (size_t)f * n + stream, sizeof(float), hipMemcpyDeviceToHost));
      rv[f - RF_q_signal] = v;
    }
  }
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

int fskhip_synth_device(fskhip_engine *e, float *d_out, size_t n, size_t pitch, uint32_t payload_len, uint64_t seed,
                        uint32_t lead_max, double amp_lo, double amp_hi, void *hip_stream) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "not configured");
  if (!d_out || pitch < n) return fail(FSKHIP_E_INVALID, "bad buffer");
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

int fskhip_demod_supported(const fskhip_engine *e) { return e && e->demod_ok ? 1 : 0; }

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

int fskhip_trace_read_pre(fskhip_engine *e, double *pre, size_t cap, size_t *n) {
  if (!e || !n) return fail(FSKHIP_E_INVALID, "null argument");
  if (!e->S.trace_n) return fail(FSKHIP_E_INVALID, "trace not enabled");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t cnt[2] = {0, 0};
  HIP_TRY(hipMemcpy(cnt, e->S.trace_n, sizeof(cnt), hipMemcpyDeviceToHost));
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
  if (!e || !n) return fail(FSKHIP_E_INVALID, "null argument");
  if (!e->S.trace_n) return fail(FSKHIP_E_INVALID, "trace not enabled");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t cnt = 0;
  HIP_TRY(hipMemcpy(&cnt, e->S.trace_n, sizeof(cnt), hipMemcpyDeviceToHost));
  size_t m = cnt < e->trace_cap ? cnt : e->trace_cap;
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
  for (uint32_t f = 0; f < (uint32_t)RF_COUNT && real_out && f < real_cap; f++) {
    if (e->precision == FSKHIP_PRECISION_F64) {
      HIP_TRY(hipMemcpy(&real_out[f], (const double *)e->S.rs + (size_t)f * n + stream, sizeof(double), hipMemcpyDeviceToHost));
    } else {
      float v = 0;
      HIP_TRY(hipMemcpy(&v, (const float *)e->S.rs + (size_t)f * n + stream, sizeof(float), hipMemcpyDeviceToHost));
      real_out[f] = (double)v;
    }
  }
  for (uint32_t f = 0; f < (uint32_t)IF_COUNT && int_out && f < int_cap; f++)
    HIP_TRY(hipMemcpy(&int_out[f], e->S.is + (size_t)f * n + stream, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (n_real) *n_real = (uint32_t)RF_COUNT;
  if (n_int) *n_int = (uint32_t)IF_COUNT;
  return FSKHIP_OK;
}

int fskhip_clock_probe_begin(fskhip_engine *e, double spin_ms) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  if (!(spin_ms > 0) || spin_ms > 10000.0) return fail(FSKHIP_E_INVALID, "spin_ms %g out of range (0, 10000]", spin_ms);
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_clock) HIP_TRY(hipMalloc((void **)&e->d_clock, 2 * sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(e->d_clock, 0, 2 * sizeof(unsigned long long), e->stream));
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, e->stream, e->d_clock, (unsigned long long)(spin_ms * 1.0e5));
  HIP_TRY(hipGetLastError());
  return FSKHIP_OK;
}
int fskhip_clock_probe_end(fskhip_engine *e, double *shader_ghz, double *covered_ms) {
  if (!e || !e->d_clock) return fail(FSKHIP_E_INVALID, "no clock probe in flight");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpy(h, e->d_clock, sizeof(h), hipMemcpyDeviceToHost));
  if (!h[1]) return fail(FSKHIP_E_HIP, "clock probe returned no ticks");
  if (shader_ghz) *shader_ghz = (double)h[0] / (double)h[1] * 0.1;
  if (covered_ms) *covered_ms = (double)h[1] * 1.0e-5;
  return FSKHIP_OK;
}

int fskhip_timing_begin(fskhip_engine *e) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  e->timing = true;
  e->ev_used = 0;
  return FSKHIP_OK;
}
int fskhip_timing_end(fskhip_engine *e, uint32_t *n_launches, double *total_ms) {
  if (!e) return fail(FSKHIP_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  e->timing = false;
  double tot = 0;
  uint32_t n = 0;
  for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
    HIP_TRY(hipEventSynchronize(e->ev[i + 1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]));
    tot += ms;
    n++;
  }
  e->ev_used = 0;
  if (n_launches) *n_launches = n;
  if (total_ms) *total_ms = tot;
  return FSKHIP_OK;
}

}  // extern "C"
