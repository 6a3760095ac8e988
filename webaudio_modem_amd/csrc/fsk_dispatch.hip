// fsk_dispatch.hip -- C ABI of libfskhip.so (include/fskhip.h): fskhip_demodulate_device / _host / _host_fmt -- the facts the choice
// of a call's kernels depends on (the choice itself: fsk_plan.h), their launches, the host-side bookkeeping, and the host forms'
// copy / compute pipeline.
#include "fsk_engine.h"
#include "fsk_launch.h"

using namespace fsk;

// everything fskhip_demodulate_device's choice of launches depends on besides its arguments (bits 8 and 16: fsk_processor.hip) --
// and every kernel argument the host advances from call to call: a captured quantum (fsk_proc.h, run_quantum) holds the launches'
// arguments by value, so a replay is the plain launch only while all of them are what they were at the capture.
//   0x1F0000 (fp64 engines)  total_samples & 31: issue_launches' P.nco_anchor, where the generic kernel re-evaluates the NCO phasor.
//                            A quantum that is no multiple of 32 samples moves it, and captures afresh on every call.
//   0x600000                 exact_split: whether the fp64 kernel runs on two waves (plan_launches, split2)
uint32_t fsk::engine_launch_key(const fskhip_engine *e) {
  const uint32_t anchor = e->precision == FSKHIP_PRECISION_F64 ? (uint32_t)(e->total_samples & 31u) : 0u;
  return (e->ds_uniform ? 1u : 0u) | (e->ds_parity << 1) | (e->force_generic ? 4u : 0u) | (e->timing.on ? 8u : 0u) |
         (e->S.trace_stream != 0xFFFFFFFFu ? 16u : 0u) | (e->gen_odd ? 64u : 0u) | (e->P.quality ? 256u : 0u) | ((uint32_t)(e->pushes & 3u) << 10) |
         ((e->blk.medium == 3u ? e->blk.med_now : e->blk.medium != 0u) ? 4096u : 0u) | ((uint32_t)e->policy << 13) | (anchor << 16) |
         ((e->exact_split & 3u) << 21);
}
// "blk_resets" = auto: tiles, and tiles the block path with resets took or would be given, of a sample of the groups since the
// last look (whatever the last completed copy brought; nothing new = the choice stands).  It wins from about one tile in six on.
void fsk::engine_refresh_kernel_choice(fskhip_engine *e) {
  if (e->blk.medium != 3u || !e->blk.h_stat) return;
  const unsigned long long hs = *e->blk.h_stat;
  const uint32_t tiles = (uint32_t)hs, rare = (uint32_t)(hs >> 32);
  const uint32_t dt = tiles - e->blk.stat_tiles, dr = rare - e->blk.stat_rare;
  if (dt == 0u) return;
  // (with hysteresis: the two kernels count slightly different things -- the plain one cannot tell whether a tile it sends
  // down its per-sample path because of a lane's own span also holds a sync candidate)
  e->blk.med_now = (double)dr >= (e->blk.med_now ? 0.10 : 0.20) * (double)dt;
  e->blk.stat_tiles = tiles; e->blk.stat_rare = rare;
}
// ... and the copy that brings the totals back, behind a launch of the four- or seven-wave kernel: behind every long call, behind
// every eighth of a run of short ones (the copy is ~3 us of the stream's time, 7 % of a 128-sample call of 65 536 streams)
static hipError_t engine_fetch_blk_stat(fskhip_engine *e, size_t n_fast, hipStream_t st) {
  if (e->blk.medium != 3u || !e->blk.h_stat || !e->S.blk_stat) return hipSuccess;
  bool fetch = n_fast >= 4096 || (++e->blk.stat_skip & 7u) == 0u;
  if (!fetch) {                                      // (a call being captured into a graph is replayed many times: it fetches)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    fetch = hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
  }
  return fetch ? hipMemcpyAsync((void *)e->blk.h_stat, e->S.blk_stat, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) : hipSuccess;
}
// the host-side counters after a call of n samples has been issued (calls = 1: a demodulateData() call of its own) or replayed
static void note_call(fskhip_engine *e, size_t n, uint32_t calls) {
  e->demodulated = true;
  e->calls += calls;
  e->total_samples += n;
  e->pushes += (e->ds_parity + n) >> 1;     // (the amplitude ring's position moves with a replayed call too)
  e->ds_parity = (e->ds_parity + (uint32_t)(n & 1)) & 1u;
}
void fsk::engine_note_replayed_call(fskhip_engine *e, size_t n) { note_call(e, n, 1u); }

// The hand-off fault word (csrc/fsk_wait.h): a wave of a multi-wave kernel got nowhere in FSK_SPIN_CAP polls of one wait and ended
// its launch early.  Sticky: the streams of that workgroup are mid-call, the engine is to be destroyed.  `blocking`: read the word
// from the device (the caller has synchronised); otherwise whatever the last completed statistics copy brought (costs nothing).
int fsk::handoff_check(fskhip_engine *e, bool blocking) {
  if (e->handoff_fault == 0u) {
    uint32_t w = 0;
    if (blocking) {
      if (e->S.blk_stat && hipMemcpy(&w, e->S.blk_stat + 2, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) w = 0;
    } else if (e->blk.h_stat) {
      w = (uint32_t)e->blk.h_stat[1];
    }
    e->handoff_fault = w;
  }
  if (e->handoff_fault != 0u)
    return fail(FSKHIP_E_HANDOFF, "a hand-off wait of a multi-wave kernel ran into its bound (fault word %u, last kernel %s): destroy the engine",
                e->handoff_fault, e->last_kernel);
  return FSKHIP_OK;
}

// ---- one demodulate call: which kernels (plan_facts -> fsk_plan.h's plan_launches), then head -> whole tiles -> tail (issue_launches) ----
namespace {
// What plan_launches reads, from the engine and the call's arguments: the one place that asks the kernel files what applies.
PlanFacts plan_facts(const fskhip_engine *e, const float *d_samples, size_t n, size_t pitch) {
  PlanFacts f{};
  f.policy = e->policy;
  f.f64 = e->precision == FSKHIP_PRECISION_F64; f.lock_step = e->ds_uniform;
  f.fast = demod_fast_applicable(e->precision, e->ds_uniform, e->P, e->S, d_samples, 0);   // (the pitch's bound is the planner's)
  f.ds_parity = e->ds_parity; f.ring_pos = (uint32_t)(e->pushes & 3u);
  f.gen_odd = e->gen_odd; f.force_generic = e->force_generic; f.diagnostics = e->S.trace_stream != 0xFFFFFFFFu || e->P.quality;
  f.n = n; f.pitch = pitch; f.ptr_low = (uint32_t)(reinterpret_cast<uintptr_t>(d_samples) & 3u);
  f.n_streams = e->n_streams; f.n_blocks = e->n_blocks; f.cus = e->cus > 0 ? (uint32_t)e->cus : 0u; f.split_cus = e->split_cus;
  f.wide_or_frac = e->P.wide || e->P.frac; f.exact_split = e->exact_split;
  if (f.f64) f.split2_lds = f.wide_or_frac ? 0 : demod_split2_lds_bytes(e->P);
  if (!f.fast) return f;   // (the whole-tile kernels' facts: lock-step fp32 engines only)
  f.blk_applicable = demod_blk_applicable(e->P); f.blk_queue = e->S.blk_q != nullptr; f.blk_lds = demod_blk_lds_bytes(e->P);
  f.blk_lanes = e->blk.lanes; f.blk_resident = e->blk.resident; f.blk_slice_tiles = e->blk.slice_tiles; f.blk_min_tiles = e->blk.min_tiles;
  f.six_applicable = demod_blk6_applicable(e->P); f.six_max_samples = demod_blk6_max_samples(); f.six_min_tiles = e->six.min_tiles;
  f.six_y_pinned = e->six.y_slots; f.six_y_default = f.six_applicable ? demod_blk6_y_slots(e->P) : 0u;
  f.pipe_lds = demod_pipe_lds_bytes(e->P);
  return f;
}

// Issues the plan's launches.  *name: what fskhip_last_kernel reports for the call -- its whole-tile kernel as the launcher named it,
// or the per-sample / generic kernel of a call without tiles.
int issue_launches(fskhip_engine *e, const LaunchPlan &pl, const DemodCall &call, const char **name) {
  if (pl.kernel == K_GENERIC) {
    e->P.nco_anchor = (uint32_t)(e->total_samples & 31u);   // (fp64: where the NCO phasor is re-evaluated; fsk_demod.hip, mix_lp)
    HIP_TRY(launch_demod(call, e->P, e->S, e->precision, e->ds_uniform, pl.split2, name));
    // the generic kernel keeps an open decimator pair's partial sums in the reference's own frame: stay with it
    // until the pair is closed
    if (call.n > 0) e->gen_odd = e->precision == FSKHIP_PRECISION_F32 && ((e->ds_parity + (uint32_t)(call.n & 1)) & 1u) != 0;
    return FSKHIP_OK;
  }
  const size_t head = pl.head, n_fast = pl.n_fast;
  const char *per_sample = "";   // the head's and the tail's kernel: the call's only where it has no tiles
  if (head) HIP_TRY(launch_demod_tail(call.sub(0, head), e->P, e->S, (int)e->ds_parity, &per_sample));
  if (!n_fast) { *name = per_sample; return FSKHIP_OK; }
  const DemodCall tiles = call.sub(head, n_fast);
  switch (pl.kernel) {
    case K_SEVEN_WAVE:
      HIP_TRY(launch_demod_blk6(tiles, e->P, e->S, e->blk.lanes, pl.y_slots, e->six.rolemap, name));
      HIP_TRY(engine_fetch_blk_stat(e, n_fast, call.stream));
      break;
    case K_FOUR_WAVE:
      HIP_TRY(launch_demod_blk(tiles, e->P, e->S, e->blk.resident, e->blk.slice_tiles, e->blk.y_slots, e->blk.lanes, pl.med, name));
      HIP_TRY(engine_fetch_blk_stat(e, n_fast, call.stream));
      break;
    case K_TWO_WAVE:
      HIP_TRY(launch_demod_pipe(tiles, e->P, e->S, name));
      break;
    default:
      HIP_TRY(launch_demod_fused(tiles, e->P, e->S, name));
  }
  const size_t done = head + n_fast;
  if (done < call.n) HIP_TRY(launch_demod_tail(call.sub(done, call.n - done), e->P, e->S, 0, &per_sample));
  return FSKHIP_OK;
}

// append_first: this launch sequence continues a call that has produced output already (a time slab of
// fskhip_demodulate_host's pipeline); count_call: it is (the first part of) a demodulateData() call of its own
int demod_device_impl(fskhip_engine *e, float *d_samples, size_t n, size_t pitch, uint8_t *d_out, size_t out_pitch, uint32_t *d_out_counts,
                      uint32_t *d_eod_counts, uint32_t flags, void *hip_stream, bool append_first, bool count_call) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "FSK demodulator not configured");
  if (!d_out_counts || (n > 0 && !d_samples) || (out_pitch > 0 && !d_out))
    return fail(FSKHIP_E_INVALID, "fskhip_demodulate_device: null buffer");
  if (pitch < n) return fail(FSKHIP_E_INVALID, "pitch %zu < n_per_stream %zu", pitch, n);
  if (!e->demod_ok) return fail(FSKHIP_E_UNSUPPORTED, "demodulator unsupported for this configuration: %s", e->demod_why.c_str());
  if (const int hrc = handoff_check(e, false)) return hrc;
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const bool wb = (flags & FSKHIP_DEMOD_WRITEBACK_AGC) != 0;
  if (const int rc = timing_open(e, st)) return rc;
  e->last_kernel = "";
  LaunchPlan pl = plan_launches(plan_facts(e, d_samples, n, pitch));
  if (pl.kernel == K_FOUR_WAVE || pl.kernel == K_SEVEN_WAVE) {   // (only then: auto's hysteresis depends on when it is consulted)
    engine_refresh_kernel_choice(e);
    pl.med = e->blk.medium == 3u ? (e->blk.med_now ? 1u : 0u) : e->blk.medium;
  }
  const char *name = "";
  if (const int rc = issue_launches(e, pl, {wb, append_first, d_samples, n, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, st}, &name)) return rc;
  e->last_kernel = name;
  if (const int rc = timing_close(e, st)) return rc;
  note_call(e, n, count_call ? 1u : 0u);
  return FSKHIP_OK;
}
// fskhip_demodulate_host (format F32, stream-major: `samples` is the caller's float*, staged as it is and written back into where
// FSKHIP_DEMOD_WRITEBACK_AGC asks) and fskhip_demodulate_host_fmt (anything else: the samples cross PCIe as they are, into a narrow
// staging slab, and fsk_samples.hip's ingest kernel widens them into the float staging tile on the compute stream).  One time pipeline:
// the same slab lengths in samples, the same two streams and events.
int demod_host_impl(fskhip_engine *e, const void *samples_, int format, int layout, size_t n, size_t pitch, uint8_t *out, size_t out_pitch,
                    uint32_t *out_counts, uint32_t *eod_counts, uint32_t flags) {
  if (!e) return fail(FSKHIP_E_NOT_CONFIGURED, "FSK demodulator not configured");
  if (!out_counts || (n > 0 && !samples_) || (out_pitch > 0 && !out)) return fail(FSKHIP_E_INVALID, "null buffer");
  const size_t S = e->n_streams;
  const bool direct = format == FSKHIP_SAMPLES_F32 && layout == FSKHIP_LAYOUT_STREAM_MAJOR;
  const bool frames = layout == FSKHIP_LAYOUT_SAMPLE_MAJOR;
  if (!frames && pitch < n) return fail(FSKHIP_E_INVALID, "pitch %zu < n_per_stream %zu", pitch, n);
  if (frames && pitch < S) return fail(FSKHIP_E_INVALID, "frame pitch %zu < n_streams %zu", pitch, S);
  const bool wb = (flags & FSKHIP_DEMOD_WRITEBACK_AGC) != 0;
  if (wb && !direct) return fail(FSKHIP_E_INVALID, "FSKHIP_DEMOD_WRITEBACK_AGC needs float samples in stream-major layout: there is nothing to write floats back into");
  HIP_TRY(hipSetDevice(e->device));
  float *const samples = direct ? (float *)const_cast<void *>(samples_) : nullptr;
  const size_t esz = sample_bytes(format);
  // slab length: ~96 MB of samples per slab, a multiple of 16 (whole tiles, even decimator parity), at least 4096
  size_t slab = ((size_t)96 << 20) / (S * sizeof(float));
  slab = slab < 4096 ? 4096 : slab;
  slab &= ~(size_t)15;
  if (e->host_slab != (size_t)-1) slab = e->host_slab & ~(size_t)15;   // fskhip_set_option("host_slab"): tests / measurements
  const bool piped = slab > 0 && n > slab + slab / 2;
  const size_t len0 = piped ? slab + slab / 2 : n;    // (the last slab of a pipelined call takes the remainder, < 1.5 slabs)
  // device copies keep a row pitch that is a multiple of 4 floats, with room for host_stage_shift's three (fsk_plan.h)
  const size_t dpitch = ((len0 + 3 + 3) & ~(size_t)3) ? ((len0 + 3 + 3) & ~(size_t)3) : 4;
  auto shift = [&]() -> size_t { return host_stage_shift(e->precision == FSKHIP_PRECISION_F64, e->ds_uniform, e->ds_parity); };
  // the narrow staging slabs: rows of 16-byte-aligned pitch (stream-major), or the slab's frames as they are (sample-major)
  const size_t npitch = frames ? pitch : (len0 + 15) & ~(size_t)15;
  const size_t nbytes = (frames ? len0 * pitch : S * npitch) * esz;
  // samples [off, off + len) of every stream: host -> staging slab b, on `st` (direct: straight into the float tile `stg`)
  auto stage_in = [&](int b, float *stg, size_t off, size_t len, hipStream_t st) -> hipError_t {
    if (direct) return hipMemcpy2DAsync(stg, dpitch * sizeof(float), samples + off, pitch * sizeof(float), len * sizeof(float), S, hipMemcpyHostToDevice, st);
    const uint8_t *from = (const uint8_t *)samples_ + off * (frames ? pitch : 1) * esz;
    if (frames) return hipMemcpyAsync(e->host.d_narrow[b], from, ((len - 1) * pitch + S) * esz, hipMemcpyHostToDevice, st);   // (the last frame: its S columns only)
    return hipMemcpy2DAsync(e->host.d_narrow[b], npitch * esz, from, pitch * esz, len * esz, S, hipMemcpyHostToDevice, st);
  };
  // ... and from there into the float tile, on the compute stream (direct: they are there already)
  auto widen = [&](int b, float *stg, size_t len) -> hipError_t {
    return direct ? hipSuccess : launch_ingest(e->host.d_narrow[b], format, layout, (uint32_t)S, len, npitch, stg, dpitch, e->host.stream);
  };
  int rc;
  if ((rc = ensure(e->host.d_samples, e->host.d_samples_cap, dpitch * S)) != FSKHIP_OK) return rc;
  if ((rc = ensure(e->host.d_out, e->host.d_out_cap, (out_pitch ? out_pitch : 1) * S)) != FSKHIP_OK) return rc;
  if (!direct && n > 0 && (rc = ensure(e->host.d_narrow[0], e->host.d_narrow_cap[0], nbytes)) != FSKHIP_OK) return rc;
  if (!piped) {
    float *stg = e->host.d_samples + shift();
    if (n > 0) {
      HIP_TRY(stage_in(0, stg, 0, n, e->host.stream));
      HIP_TRY(widen(0, stg, n));
    }
    rc = demod_device_impl(e, stg, n, dpitch, e->host.d_out, out_pitch, e->host.d_counts, e->host.d_eod, flags, e->host.stream, false, true);
    if (rc != FSKHIP_OK) return rc;
    if (wb && n > 0)
      HIP_TRY(hipMemcpy2DAsync(samples, pitch * sizeof(float), stg, dpitch * sizeof(float), n * sizeof(float), S,
                               hipMemcpyDeviceToHost, e->host.stream));
  } else {
    if ((rc = ensure(e->host.d_samples2, e->host.d_samples2_cap, dpitch * S)) != FSKHIP_OK) return rc;
    if (!direct && (rc = ensure(e->host.d_narrow[1], e->host.d_narrow_cap[1], nbytes)) != FSKHIP_OK) return rc;
    if (!e->host.copy_stream) {
      HIP_TRY(hipStreamCreateWithFlags(&e->host.copy_stream, hipStreamNonBlocking));
      for (int i = 0; i < 2; i++) {
        HIP_TRY(hipEventCreateWithFlags(&e->host.ev_copied[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->host.ev_used_up[i], hipEventDisableTiming));
      }
    }
    // on a failure inside the pipeline, let what is in flight on both streams finish before the caller's buffers go away
#define PIPE_TRY(expr) HIP_TRY_AS(expr, #expr, false, ((void)hipStreamSynchronize(e->host.copy_stream), (void)hipStreamSynchronize(e->host.stream)))
    float *buf[2] = {e->host.d_samples, e->host.d_samples2};
    size_t off = 0;
    for (size_t j = 0; off < n; j++) {
      // the last slab takes the remainder (up to 1.5 slabs would not be worth another round trip)
      const size_t len = (n - off > slab + slab / 2) ? slab : n - off;
      if (len + 3 > dpitch) return fail(FSKHIP_E_INVALID, "internal: slab %zu exceeds staging pitch %zu", len, dpitch);
      const int b = (int)(j & 1);
      float *stg = buf[b] + shift();               // (the parity at this slab's start: slabs are multiples of 16 samples)
      if (j >= 2) PIPE_TRY(hipStreamWaitEvent(e->host.copy_stream, e->host.ev_used_up[b], 0));   // its previous user has finished
      PIPE_TRY(stage_in(b, stg, off, len, e->host.copy_stream));
      PIPE_TRY(hipEventRecord(e->host.ev_copied[b], e->host.copy_stream));
      PIPE_TRY(hipStreamWaitEvent(e->host.stream, e->host.ev_copied[b], 0));
      PIPE_TRY(widen(b, stg, len));
      rc = demod_device_impl(e, stg, len, dpitch, e->host.d_out, out_pitch, e->host.d_counts, e->host.d_eod, flags, e->host.stream,
                             /*append_first=*/j > 0, /*count_call=*/j == 0);
      if (rc != FSKHIP_OK) { (void)hipStreamSynchronize(e->host.copy_stream); (void)hipStreamSynchronize(e->host.stream); return rc; }
      if (wb)
        PIPE_TRY(hipMemcpy2DAsync(samples + off, pitch * sizeof(float), stg, dpitch * sizeof(float), len * sizeof(float), S,
                                 hipMemcpyDeviceToHost, e->host.stream));
      PIPE_TRY(hipEventRecord(e->host.ev_used_up[b], e->host.stream));
      off += len;
    }
#undef PIPE_TRY
  }
  if (out_pitch > 0) HIP_TRY(hipMemcpyAsync(out, e->host.d_out, out_pitch * S, hipMemcpyDeviceToHost, e->host.stream));
  HIP_TRY(hipMemcpyAsync(out_counts, e->host.d_counts, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, e->host.stream));
  if (eod_counts) HIP_TRY(hipMemcpyAsync(eod_counts, e->host.d_eod, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, e->host.stream));
  HIP_TRY(hipStreamSynchronize(e->host.stream));
  if (e->host.copy_stream) HIP_TRY(hipStreamSynchronize(e->host.copy_stream));
  if (const int hrc = handoff_check(e, true)) return hrc;
  for (size_t s = 0; s < S; s++)
    if (out_counts[s] > out_pitch) return fail(FSKHIP_E_OVERFLOW, "stream %zu produced %u bytes, slab holds %zu", s, out_counts[s], out_pitch);
  return FSKHIP_OK;
}
}  // namespace

extern "C" {
int fskhip_demodulate_device(fskhip_engine *e, float *d_samples, size_t n, size_t pitch, uint8_t *d_out, size_t out_pitch,
                             uint32_t *d_out_counts, uint32_t *d_eod_counts, uint32_t flags, void *hip_stream) {
  return demod_device_impl(e, d_samples, n, pitch, d_out, out_pitch, d_out_counts, d_eod_counts, flags, hip_stream, false, true);
}
// Host buffers in, bytes out.  A call longer than one time slab is a two-buffer pipeline over TIME: slab j+1 crosses PCIe
// on the copy stream while slab j is demodulated on the compute stream.  Cutting along time needs no sub-batch launches,
// and the engine gives the same bytes for any cut (the reference is a streaming state machine, fsk.ts:190-222).  The
// copies only overlap if `samples` is page-locked (fskhip_host_alloc, or any pinned buffer of the caller); with pageable
// memory the runtime stages each copy itself and the pipeline degrades gracefully to what one big copy costs.
int fskhip_demodulate_host(fskhip_engine *e, float *samples, size_t n, size_t pitch, uint8_t *out, size_t out_pitch,
                           uint32_t *out_counts, uint32_t *eod_counts, uint32_t flags) {
  return demod_host_impl(e, samples, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_STREAM_MAJOR, n, pitch, out, out_pitch, out_counts, eod_counts, flags);
}
// ... and the same for samples in any capture format and layout (include/fskhip.h), read only
int fskhip_demodulate_host_fmt(fskhip_engine *e, const void *samples, int format, int layout, size_t n, size_t src_pitch, uint8_t *out,
                               size_t out_pitch, uint32_t *out_counts, uint32_t *eod_counts, uint32_t flags) {
  if (const int rc = check_sample_format("fskhip_demodulate_host_fmt", format, layout)) return rc;
  return demod_host_impl(e, samples, format, layout, n, src_pitch, out, out_pitch, out_counts, eod_counts, flags);
}
}  // extern "C"
