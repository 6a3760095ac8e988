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

#include "fsk_processor_rate_host.h"
#include "fsk_processor_rate_plan.h"
#include "fsk_resampler.h"

using namespace fsk;

namespace {

const HandleWords kWords = {{"up", "down"}, "resamples"};

// the launches of one quantum, in stream order: interpolator, the demodulator's, bookkeeping / TX (/ decimator); a handle's history
// buffers change places behind the launch that wrote the other one
int launch_quantum_rate(const char *who, fskhip_processor *p, const Side &in, size_t fin_pitch, const Side &out, bool fused, size_t ftx_pitch, uint32_t flags,
                        hipStream_t st) {
  if (in.ptr) {
    RateHost *const u = in.r;
    if (in.n) {
      if (const int rc = launch_failed(who, launch_resample_up(u->precision, in.ptr, in.format, in.layout, p->S, in.n, in.pitch, p->d_fin, fin_pitch, u->L,
                                                               u->n_taps, u->taps(), u->hist[u->cur], u->hist[u->cur ^ 1], st), p->S, in.n)) return rc;
      if (u->H) u->cur ^= 1;
    }
    if (const int rc = fskhip_demodulate_device(p->e, p->d_fin, in.n * u->L, fin_pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, st)) return rc;
  }
  const bool clear = (flags & FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE) != 0;
  RateHost *const d = out.r;
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
  const char *const tx = !(out.ptr && out.n) ? kTxNone : fused ? kTxRate : kTxRatePair;
  // plainly, whatever FSKHIP_PROC_GRAPH says: the handles' history pointers change from call to call
  return run_quantum_tx(p, tx, {nullptr, n_hi, fin_pitch, nullptr, out.n, out.pitch, flags & ~FSKHIP_PROC_GRAPH, st, 0u}, in.ptr != nullptr,
                     [&](uint32_t f) { return launch_quantum_rate(who, p, in, fin_pitch, out, fused, ftx_pitch, f, st); });
}

}  // namespace

extern "C" {

int fskhip_processor_process_rate_device(fskhip_processor *p, fskhip_resampler *up, fskhip_resampler *down, const void *d_in, int in_format, int in_layout,
                                         size_t n_in, size_t in_pitch, void *d_out, int out_format, int out_layout, size_t n_out, size_t out_pitch,
                                         uint32_t flags, void *hip_stream) {
  static const char who[] = "fskhip_processor_process_rate_device";
  const Side in{d_in, in_format, in_layout, n_in, in_pitch, up}, out{d_out, out_format, out_layout, n_out, out_pitch, down};
  if (const int rc = rate_refusal(who, kWords, p, in, "d_in", out, "d_out")) return rc;
  return process_rate_device(who, p, in, out, flags, (hipStream_t)hip_stream);
}

// Host memory either way: the low rate samples cross PCIe as they are, staged as fskhip_processor_process_fmt_host stages its own.
int fskhip_processor_process_rate_host(fskhip_processor *p, fskhip_resampler *up, fskhip_resampler *down, const void *in_, int in_format, int in_layout,
                                       size_t n_in, size_t in_pitch, void *out_, int out_format, int out_layout, size_t n_out, size_t out_pitch,
                                       uint32_t flags) {
  static const char who[] = "fskhip_processor_process_rate_host";
  const Side in{in_, in_format, in_layout, n_in, in_pitch, up}, out{out_, out_format, out_layout, n_out, out_pitch, down};
  if (const int rc = rate_refusal(who, kWords, p, in, "in", out, "out")) return rc;
  return rate_host_quantum(p, in, out, [&](const Side &d_in, const Side &d_out) { return process_rate_device(who, p, d_in, d_out, flags, p->stream); });
}

}  // extern "C"
