// fsk_processor_rate.hip -- fskhip_processor_process_rate_* (include/fskhip_next.h): the FSKProcessor quantum of fsk_processor.hip with
// both sides at a trunk's low rate, in a capture format and layout, through two fskhip_resampler handles (fsk_resample.hip).
//   RX   one launch_resample_up writes the quantum, interpolated, into the float tile kept with the processor (d_fin) in place of
//        fsk_processor_fmt.hip's ingest launch; the demodulator launches and the ring puts are fskhip_processor_process_device's on
//        that tile.
//   TX   fsk_mod.hip's processor_io_rate_kernel: generator, decimator and encoder in one launch, the high rate floats in LDS.  A
//        decimator whose delay line does not fit, and interleaved frames (fsk_processor_rate_plan.h), take the two launches that
//        kernel replaces: processor_io_kernel into a float tile kept with the processor (d_ftx), then launch_resample_down.
// Either way every word of processor, engine and handle state ends as the chain of the three existing calls leaves it.
#include <hip/hip_runtime.h>

#include "fsk_engine.h"
#include "fsk_launch.h"
#include "fsk_plan.h"
#include "fsk_proc.h"
#include "fsk_processor_rate_plan.h"
#include "fsk_resampler.h"

using namespace fsk;

namespace {

struct Side {
  const void *ptr; int format, layout; size_t n, pitch; fskhip_resampler *r;
  bool frames() const { return layout == FSKHIP_LAYOUT_SAMPLE_MAJOR; }
};

// a side's handle: there, of the side's direction, and the processor's in streams and device
int handle_refusal(const char *who, const fskhip_processor *p, const fskhip_resampler *r, int direction) {
  const char *const name = direction == FSKHIP_RESAMPLE_UP ? "up" : "down";
  if (!r) return fail(FSKHIP_E_INVALID, "%s: null %s handle", who, name);
  if (r->direction != direction) return fail(FSKHIP_E_INVALID, "%s: the %s handle resamples %s", who, name, r->direction == FSKHIP_RESAMPLE_UP ? "up" : "down");
  if (r->S != p->S) return fail(FSKHIP_E_INVALID, "%s: the %s handle has %u streams, the processor %u", who, name, r->S, p->S);
  if (r->device != p->device) return fail(FSKHIP_E_INVALID, "%s: the %s handle is on device %d, the processor on %d", who, name, r->device, p->device);
  return FSKHIP_OK;
}

// what both forms refuse before any device call, in the header's order; in_name / out_name: the arguments as the form calls them
int rate_refusal(const char *who, const fskhip_processor *p, const Side &in, const char *in_name, const Side &out, const char *out_name) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (const int rc = check_sample_format(who, in.format, in.layout)) return rc;
  if (const int rc = check_sample_format(who, out.format, out.layout)) return rc;
  if (in.ptr)
    if (const int rc = handle_refusal(who, p, in.r, FSKHIP_RESAMPLE_UP)) return rc;
  if (out.ptr)
    if (const int rc = handle_refusal(who, p, out.r, FSKHIP_RESAMPLE_DOWN)) return rc;
  if (in.ptr && !in.frames() && in.pitch < in.n) return fail(FSKHIP_E_INVALID, "in_pitch %zu < n_in %zu", in.pitch, in.n);
  if (in.ptr && in.frames() && in.pitch < p->S) return fail(FSKHIP_E_INVALID, "in frame pitch %zu < n_streams %u", in.pitch, p->S);
  if (out.ptr && !out.frames() && out.pitch < out.n) return fail(FSKHIP_E_INVALID, "out_pitch %zu < n_out %zu", out.pitch, out.n);
  if (out.ptr && out.frames() && out.pitch < p->S) return fail(FSKHIP_E_INVALID, "out frame pitch %zu < n_streams %u", out.pitch, p->S);
  if ((reinterpret_cast<uintptr_t>(in.ptr) & (sample_bytes(in.format) - 1u)) != 0) return fail(FSKHIP_E_INVALID, "%s is not aligned to its element size", in_name);
  if ((reinterpret_cast<uintptr_t>(out.ptr) & (sample_bytes(out.format) - 1u)) != 0) return fail(FSKHIP_E_INVALID, "%s is not aligned to its element size", out_name);
  return FSKHIP_OK;
}

int launch_failed(const char *who, hipError_t err, uint32_t n_streams, size_t n) {
  if (err == hipErrorInvalidValue) return fail(FSKHIP_E_INVALID, "%s: %u streams x %zu samples are more workgroups than one launch takes", who, n_streams, n);
  HIP_TRY(err);
  return FSKHIP_OK;
}

// the launches of one quantum, in stream order: interpolator, the demodulator's, bookkeeping / TX (/ decimator); a handle's history
// buffers change places behind the launch that wrote the other one
int launch_quantum_rate(const char *who, fskhip_processor *p, const Side &in, size_t fin_pitch, const Side &out, bool fused, size_t ftx_pitch, uint32_t flags,
                        hipStream_t st) {
  if (in.ptr) {
    fskhip_resampler *const u = in.r;
    if (in.n) {
      if (const int rc = launch_failed(who, launch_resample_up(u->precision, in.ptr, in.format, in.layout, p->S, in.n, in.pitch, p->d_fin, fin_pitch, u->L,
                                                               u->n_taps, u->taps(), u->hist[u->cur], u->hist[u->cur ^ 1], st), p->S, in.n)) return rc;
      if (u->H) u->cur ^= 1;
    }
    if (const int rc = fskhip_demodulate_device(p->e, p->d_fin, in.n * u->L, fin_pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, st)) return rc;
  }
  const bool clear = (flags & FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE) != 0;
  fskhip_resampler *const d = out.r;
  if (!out.ptr || out.n == 0) {   // no TX side: the ring puts alone
    HIP_TRY(launch_processor_io(p->e->M, p->e->S.coef, p->T, p->d_bytes, p->bytes_pitch, p->d_counts, in.ptr != nullptr, nullptr, 0, 0, clear, st));
    return FSKHIP_OK;
  }
  if (fused) {
    HIP_TRY(launch_processor_io_rate(p->e->M, p->e->S.coef, p->T, p->d_bytes, p->bytes_pitch, p->d_counts, in.ptr != nullptr, const_cast<void *>(out.ptr), out.format,
                                     out.layout, out.n, out.pitch, clear, d->precision, d->L, d->n_taps, d->taps(), d->hist[d->cur], d->hist[d->cur ^ 1], st));
  } else {
    HIP_TRY(launch_processor_io(p->e->M, p->e->S.coef, p->T, p->d_bytes, p->bytes_pitch, p->d_counts, in.ptr != nullptr, p->d_ftx, out.n * d->L, ftx_pitch, clear, st));
    if (const int rc = launch_failed(who, launch_resample_down(d->precision, p->d_ftx, out.n, ftx_pitch, nullptr, p->S, const_cast<void *>(out.ptr), out.format,
                                                               out.layout, out.pitch, d->L, d->n_taps, d->taps(), d->hist[d->cur], d->hist[d->cur ^ 1], st), p->S,
                                     out.n)) return rc;
  }
  if (d->H) d->cur ^= 1;
  return FSKHIP_OK;
}

int process_rate_device(const char *who, fskhip_processor *p, const Side &in, const Side &out, uint32_t flags, hipStream_t st) {
  p->used = true;
  if (in.ptr && !fskhip_demod_supported(p->e)) {
    // let the engine produce its own loud message
    return fskhip_demodulate_device(p->e, (float *)const_cast<void *>(in.ptr), in.n, in.pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, st);
  }
  HIP_TRY(hipSetDevice(p->device));
  const size_t n_hi = in.ptr ? in.n * in.r->L : 0, n_ho = out.ptr ? out.n * out.r->L : 0;
  const size_t fin_pitch = n_hi ? (n_hi + 3) & ~(size_t)3 : 4, ftx_pitch = n_ho ? (n_ho + 3) & ~(size_t)3 : 4;   // rows on 16-byte boundaries
  const bool fused = out.ptr && processor_rate_plan(out.r->L, out.r->n_taps, (uint32_t)sample_bytes(out.format), !out.frames()).fused;
  if (in.ptr) {  // byte slab and float tile of this quantum
    if (const int rc = grow_byte_slab(p, n_hi)) return rc;
    if (const int rc = grow_for_quantum(p, p->d_fin, p->d_fin_cap, fin_pitch * p->S)) return rc;
  }
  if (out.ptr && out.n && !fused)
    if (const int rc = grow_for_quantum(p, p->d_ftx, p->d_ftx_cap, ftx_pitch * p->S)) return rc;
  // plainly, whatever FSKHIP_PROC_GRAPH says: the handles' history pointers change from call to call
  return run_quantum(p, {nullptr, n_hi, fin_pitch, nullptr, out.n, out.pitch, flags & ~FSKHIP_PROC_GRAPH, st, 0u}, in.ptr != nullptr,
                     [&](uint32_t f) { return launch_quantum_rate(who, p, in, fin_pitch, out, fused, ftx_pitch, f, st); });
}

}  // namespace

extern "C" {

int fskhip_processor_process_rate_device(fskhip_processor *p, fskhip_resampler *up, fskhip_resampler *down, const void *d_in, int in_format, int in_layout,
                                         size_t n_in, size_t in_pitch, void *d_out, int out_format, int out_layout, size_t n_out, size_t out_pitch,
                                         uint32_t flags, void *hip_stream) {
  static const char who[] = "fskhip_processor_process_rate_device";
  const Side in{d_in, in_format, in_layout, n_in, in_pitch, up}, out{d_out, out_format, out_layout, n_out, out_pitch, down};
  if (const int rc = rate_refusal(who, p, in, "d_in", out, "d_out")) return rc;
  return process_rate_device(who, p, in, out, flags, (hipStream_t)hip_stream);
}

// Host memory either way: the low rate samples cross PCIe as they are, staged as fskhip_processor_process_fmt_host stages its own.
int fskhip_processor_process_rate_host(fskhip_processor *p, fskhip_resampler *up, fskhip_resampler *down, const void *in_, int in_format, int in_layout,
                                       size_t n_in, size_t in_pitch, void *out_, int out_format, int out_layout, size_t n_out, size_t out_pitch,
                                       uint32_t flags) {
  static const char who[] = "fskhip_processor_process_rate_host";
  if (const int rc = rate_refusal(who, p, {in_, in_format, in_layout, n_in, in_pitch, up}, "in", {out_, out_format, out_layout, n_out, out_pitch, down}, "out"))
    return rc;
  HIP_TRY(hipSetDevice(p->device));
  const size_t S = p->S, isz = sample_bytes(in_format), osz = sample_bytes(out_format);
  const bool in_frames = in_layout == FSKHIP_LAYOUT_SAMPLE_MAJOR, out_frames = out_layout == FSKHIP_LAYOUT_SAMPLE_MAJOR;
  const size_t d_in_pitch = in_frames ? in_pitch : ((n_in * isz + 15) & ~(size_t)15) / isz;
  const size_t in_bytes = in_frames ? (n_in ? ((n_in - 1) * in_pitch + S) * isz : 0) : S * d_in_pitch * isz;   // (the last frame: its S columns only)
  const EgressStage g = egress_stage(S, n_out, osz, out_frames);
  int rc;
  if (in_ && (rc = grow_for_quantum(p, p->d_nin, p->d_nin_cap, in_bytes ? in_bytes : 16)) != FSKHIP_OK) return rc;
  if (out_ && (rc = grow_for_quantum(p, p->d_nout, p->d_nout_cap, g.bytes ? g.bytes : 16)) != FSKHIP_OK) return rc;
  if (in_ && n_in) {
    if (in_frames) HIP_TRY(hipMemcpyAsync(p->d_nin, in_, in_bytes, hipMemcpyHostToDevice, p->stream));
    else HIP_TRY(hipMemcpy2DAsync(p->d_nin, d_in_pitch * isz, in_, in_pitch * isz, n_in * isz, S, hipMemcpyHostToDevice, p->stream));
  }
  const Side in{in_ ? p->d_nin : nullptr, in_format, in_layout, n_in, d_in_pitch ? d_in_pitch : 16 / isz, up};
  const Side out{out_ ? p->d_nout : nullptr, out_format, out_layout, n_out, g.npitch ? g.npitch : 16 / osz, down};
  if ((rc = process_rate_device(who, p, in, out, flags, p->stream)) != FSKHIP_OK) return rc;
  if (out_ && n_out) HIP_TRY(hipMemcpy2DAsync(out_, out_pitch * osz, p->d_nout, g.npitch * osz, g.row_bytes, g.rows, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return FSKHIP_OK;
}

}  // extern "C"
