// fsk_processor_ratecvt.hip -- fskhip_processor_process_ratecvt_* (include/fskhip_next.h): the FSKProcessor quantum of
// fsk_processor.hip with both sides at a converter's outer rate (44.1 kHz either side of a 48 kHz engine), in a capture format and
// layout, through two fskhip_ratecvt handles (fsk_ratecvt.hip).
//   RX   one launch_ratecvt (capture) writes the quantum, converted, into the float tile kept with the processor (d_fin) in place
//        of fsk_processor_fmt.hip's ingest launch; the demodulator launches and the ring puts are fskhip_processor_process_device's
//        on that tile.
//   TX   fsk_mod.hip's processor_io_ratecvt_kernel: generator, converter and encoder in one launch, the engine rate floats in LDS.
//        A converter whose delay line does not fit, and interleaved frames (fsk_processor_rate_plan.h: processor_ratecvt_plan),
//        take the two launches that kernel replaces: processor_io_kernel into a float tile kept with the processor (d_ftx), then
//        launch_ratecvt (playback).
// Either way every word of processor, engine and handle state ends as the chain of the three existing calls leaves it.  What the
// call shares with fsk_processor_rate.hip is fsk_processor_rate_host.h's.
// fskhip_processor_process_ratecvt_any_* are the same quantum with sides of any length, from the handles' positions
// (fsk_ratecvt_plan.h): the engine's counts are the handles' own, and a side without engine samples is left out of the processor's
// part.  TX takes the same choice: the fused kernel's ANY form from the playback handle's position (fsk_processor_rate_plan.h:
// processor_ratecvt_start) -- its whole-period form for whole periods from position 0 --, the two launches for frames, for a
// converter beyond the delay line and under FSKHIP_PROC_RATECVT_PAIR.  fskhip_processor_last_tx_kernel says which.
#include <hip/hip_runtime.h>

#include "fsk_processor_rate_host.h"
#include "fsk_processor_rate_plan.h"
#include "fsk_ratecvt.h"
#include "fsk_ratecvt_plan.h"

using namespace fsk;

namespace {

const HandleWords kWords = {{"capture", "playback"}, "converts for"};

fskhip_ratecvt *cvt(const Side &side) { return static_cast<fskhip_ratecvt *>(side.r); }

// rate_refusal, and behind it the two counts: whole periods of the side's handle, from a period boundary; `any`: any counts, but
// an n_out that the playback handle can write from where it is
int ratecvt_refusal(const char *who, bool any, const fskhip_processor *p, const Side &in, const char *in_name, const Side &out, const char *out_name) {
  if (const int rc = rate_refusal(who, kWords, p, in, in_name, out, out_name)) return rc;
  if (any) {
    if (out.ptr) {
      const fskhip_ratecvt *const d = cvt(out);
      const size_t n_ho = ratecvt_in_count_any(d->L, d->M, d->pos, out.n), above = ratecvt_out_count_any(d->L, d->M, d->pos, n_ho);
      if (above != out.n)
        return fail(FSKHIP_E_INVALID, "%s: the playback handle at position %u cannot write n_out %zu: %zu engine samples give %zu, %zu give %zu", who, d->pos, out.n,
                    n_ho - 1, ratecvt_out_count_any(d->L, d->M, d->pos, n_ho - 1), n_ho, above);
    }
    return FSKHIP_OK;
  }
  if (in.ptr && in.n % cvt(in)->M != 0)
    return fail(FSKHIP_E_INVALID, "%s: n_in %zu is not a multiple of the capture handle's down factor %u", who, in.n, cvt(in)->M);
  if (out.ptr && out.n % cvt(out)->L != 0)
    return fail(FSKHIP_E_INVALID, "%s: n_out %zu is not a multiple of the playback handle's up factor %u", who, out.n, cvt(out)->L);
  for (const Side *side : {&in, &out})
    if (side->ptr && cvt(*side)->pos != 0)
      return fail(FSKHIP_E_INVALID, "%s: the %s handle is at position %u, not at a period boundary", who, kWords.name[side == &out], cvt(*side)->pos);
  return FSKHIP_OK;
}

// the launches of one quantum, in stream order: capture converter, the demodulator's, bookkeeping / TX (/ playback converter); a
// handle's history buffers change places, and its position moves on, behind the launch that wrote the other one.  n_hi / n_ho: the
// engine's samples in and out; rx: the processor has an input side.
int launch_quantum_ratecvt(const char *who, fskhip_processor *p, const Side &in, bool rx, size_t n_hi, size_t fin_pitch, const Side &out, size_t n_ho, bool fused,
                           size_t ftx_pitch, uint32_t flags, hipStream_t st) {
  if (in.ptr) {
    fskhip_ratecvt *const c = cvt(in);
    if (in.n) {
      if (const int rc = launch_failed(who, launch_ratecvt(FSKHIP_RATECVT_CAPTURE, c->precision, in.ptr, in.pitch, nullptr, p->d_fin, fin_pitch, in.format,
                                                           in.layout, p->S, c->pos, in.n, c->L, c->M, c->n_taps, c->taps(), c->d_table, c->hist[c->cur],
                                                           c->hist[c->cur ^ 1], st),
                                       p->S, in.n)) return rc;
      if (c->H) c->cur ^= 1;
      c->pos = ratecvt_next_position(c->M, c->pos, in.n);
    }
    if (rx)
      if (const int rc = fskhip_demodulate_device(p->e, p->d_fin, n_hi, fin_pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, st)) return rc;
  }
  const bool clear = (flags & FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE) != 0;
  if (!out.ptr || out.n == 0) {   // no TX side: the ring puts alone
    HIP_TRY(launch_processor_io(p->e->M, p->e->S.coef, p->T, p->d_bytes, p->bytes_pitch, p->d_counts, rx, nullptr, 0, 0, clear, st));
    return FSKHIP_OK;
  }
  fskhip_ratecvt *const d = cvt(out);
  if (fused) {
    HIP_TRY(launch_processor_io_ratecvt(p->e->M, p->e->S.coef, p->T, p->d_bytes, p->bytes_pitch, p->d_counts, rx, const_cast<void *>(out.ptr),
                                        out.format, out.layout, out.n, out.pitch, clear, d->precision, d->L, d->M, d->pos, n_ho, d->n_taps, d->taps(),
                                        d->hist[d->cur], d->hist[d->cur ^ 1], st));
  } else {
    HIP_TRY(launch_processor_io(p->e->M, p->e->S.coef, p->T, p->d_bytes, p->bytes_pitch, p->d_counts, rx, p->d_ftx, n_ho, ftx_pitch, clear, st));
    if (const int rc = launch_failed(who, launch_ratecvt(FSKHIP_RATECVT_PLAYBACK, d->precision, p->d_ftx, ftx_pitch, nullptr, const_cast<void *>(out.ptr),
                                                         out.pitch, out.format, out.layout, p->S, d->pos, n_ho, d->L, d->M, d->n_taps, d->taps(), d->d_table,
                                                         d->hist[d->cur], d->hist[d->cur ^ 1], st), p->S, n_ho)) return rc;
  }
  if (d->H) d->cur ^= 1;
  d->pos = ratecvt_next_position(d->M, d->pos, n_ho);
  return FSKHIP_OK;
}

int process_ratecvt_device(const char *who, bool any, fskhip_processor *p, const Side &in, const Side &out, uint32_t flags, hipStream_t st) {
  p->used = true;
  if (in.ptr && !fskhip_demod_supported(p->e)) {
    // let the engine produce its own loud message
    return fskhip_demodulate_device(p->e, (float *)const_cast<void *>(in.ptr), in.n, in.pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, st);
  }
  HIP_TRY(hipSetDevice(p->device));
  // (from position 0 and in whole periods n_hi is n_in / Mc * Lc; whole periods of output take whole periods of engine samples,
  // n_out / Lp * Mp, where any length takes the fewest that write n_out)
  const size_t n_hi = in.ptr ? ratecvt_out_count_any(cvt(in)->L, cvt(in)->M, cvt(in)->pos, in.n) : 0;
  const size_t n_ho = !out.ptr ? 0 : any ? ratecvt_in_count_any(cvt(out)->L, cvt(out)->M, cvt(out)->pos, out.n) : out.n / cvt(out)->L * cvt(out)->M;
  const bool rx = in.ptr && (!any || n_hi > 0);
  const size_t fin_pitch = n_hi ? (n_hi + 3) & ~(size_t)3 : 4, ftx_pitch = n_ho ? (n_ho + 3) & ~(size_t)3 : 4;   // rows on 16-byte boundaries
  const bool fused = out.ptr && !(flags & FSKHIP_PROC_RATECVT_PAIR) &&
                     processor_ratecvt_plan(out.r->L, out.r->n_taps, (uint32_t)sample_bytes(out.format), !out.frames()).fused;
  if (in.ptr) {  // byte slab and float tile of this quantum
    if (rx)
      if (const int rc = grow_byte_slab(p, n_hi)) return rc;
    if (const int rc = grow_for_quantum(p, p->d_fin, p->d_fin_cap, fin_pitch * p->S)) return rc;
  }
  if (out.ptr && out.n && !fused)
    if (const int rc = grow_for_quantum(p, p->d_ftx, p->d_ftx_cap, ftx_pitch * p->S)) return rc;
  // (the pair's second launch chooses as launch_ratecvt does; the fused kernel as its launcher does)
  const bool tx_any = out.ptr && (fused ? processor_ratecvt_any(cvt(out)->L, cvt(out)->M, cvt(out)->pos, out.n, n_ho) : cvt(out)->pos != 0 || n_ho % cvt(out)->M != 0);
  const char *const tx = !(out.ptr && out.n) ? kTxNone : fused ? (tx_any ? kTxRatecvtAny : kTxRatecvt) : tx_any ? kTxRatecvtAnyPair : kTxRatecvtPair;
  // plainly, whatever FSKHIP_PROC_GRAPH says: the handles' history pointers change from call to call
  return run_quantum_tx(p, tx, {nullptr, n_hi, fin_pitch, nullptr, out.n, out.pitch, flags & ~FSKHIP_PROC_GRAPH, st, 0u}, rx,
                     [&](uint32_t f) { return launch_quantum_ratecvt(who, p, in, rx, n_hi, fin_pitch, out, n_ho, fused, ftx_pitch, f, st); });
}

}  // namespace

extern "C" {

int fskhip_processor_process_ratecvt_device(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback, const void *d_in, int in_format,
                                            int in_layout, size_t n_in, size_t in_pitch, void *d_out, int out_format, int out_layout, size_t n_out,
                                            size_t out_pitch, uint32_t flags, void *hip_stream) {
  static const char who[] = "fskhip_processor_process_ratecvt_device";
  const Side in{d_in, in_format, in_layout, n_in, in_pitch, capture}, out{d_out, out_format, out_layout, n_out, out_pitch, playback};
  if (const int rc = ratecvt_refusal(who, false, p, in, "d_in", out, "d_out")) return rc;
  return process_ratecvt_device(who, false, p, in, out, flags, (hipStream_t)hip_stream);
}

int fskhip_processor_process_ratecvt_any_device(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback, const void *d_in, int in_format,
                                                int in_layout, size_t n_in, size_t in_pitch, void *d_out, int out_format, int out_layout, size_t n_out,
                                                size_t out_pitch, uint32_t flags, void *hip_stream) {
  static const char who[] = "fskhip_processor_process_ratecvt_any_device";
  const Side in{d_in, in_format, in_layout, n_in, in_pitch, capture}, out{d_out, out_format, out_layout, n_out, out_pitch, playback};
  if (const int rc = ratecvt_refusal(who, true, p, in, "d_in", out, "d_out")) return rc;
  return process_ratecvt_device(who, true, p, in, out, flags, (hipStream_t)hip_stream);
}

// Host memory either way: the outer rate samples cross PCIe as they are, staged as fskhip_processor_process_fmt_host stages its own.
int fskhip_processor_process_ratecvt_host(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback, const void *in_, int in_format,
                                          int in_layout, size_t n_in, size_t in_pitch, void *out_, int out_format, int out_layout, size_t n_out,
                                          size_t out_pitch, uint32_t flags) {
  static const char who[] = "fskhip_processor_process_ratecvt_host";
  const Side in{in_, in_format, in_layout, n_in, in_pitch, capture}, out{out_, out_format, out_layout, n_out, out_pitch, playback};
  if (const int rc = ratecvt_refusal(who, false, p, in, "in", out, "out")) return rc;
  return rate_host_quantum(p, in, out, [&](const Side &d_in, const Side &d_out) { return process_ratecvt_device(who, false, p, d_in, d_out, flags, p->stream); });
}

int fskhip_processor_process_ratecvt_any_host(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback, const void *in_, int in_format,
                                              int in_layout, size_t n_in, size_t in_pitch, void *out_, int out_format, int out_layout, size_t n_out,
                                              size_t out_pitch, uint32_t flags) {
  static const char who[] = "fskhip_processor_process_ratecvt_any_host";
  const Side in{in_, in_format, in_layout, n_in, in_pitch, capture}, out{out_, out_format, out_layout, n_out, out_pitch, playback};
  if (const int rc = ratecvt_refusal(who, true, p, in, "in", out, "out")) return rc;
  return rate_host_quantum(p, in, out, [&](const Side &d_in, const Side &d_out) { return process_ratecvt_device(who, true, p, d_in, d_out, flags, p->stream); });
}

}  // extern "C"
