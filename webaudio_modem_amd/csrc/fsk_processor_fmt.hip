// fsk_processor_fmt.hip -- fskhip_processor_process_fmt_* (include/fskhip_next.h): the FSKProcessor quantum of fsk_processor.hip with
// either side in a capture format and layout (include/fskhip.h: FSKHIP_SAMPLES_* / FSKHIP_LAYOUT_*).
//   RX   one ingest launch (fsk_samples.hip) widens the quantum into a float tile kept with the processor; the demodulator launches
//        and the ring puts are those of fskhip_processor_process_device on that tile, so every state word ends as it does there.
//   TX   fsk_mod.hip's format-writing io kernel: the codes are stored by the kernel that generates the samples.
// A side that is float32 stream-major takes the float path of that side; both of them: the call IS fskhip_processor_process_*.
#include <hip/hip_runtime.h>

#include "fsk_engine.h"
#include "fsk_launch.h"
#include "fsk_plan.h"
#include "fsk_proc.h"

using namespace fsk;

namespace {

struct Side {
  const void *ptr; int format, layout; size_t n, pitch;
  bool floats() const { return format == FSKHIP_SAMPLES_F32 && layout == FSKHIP_LAYOUT_STREAM_MAJOR; }
  bool frames() const { return layout == FSKHIP_LAYOUT_SAMPLE_MAJOR; }
};

// what both forms refuse before any device call, in the header's order; in_name / out_name: the arguments as the form calls them
int fmt_refusal(const char *who, const fskhip_processor *p, const Side &in, const char *in_name, const Side &out, const char *out_name) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (const int rc = check_sample_format(who, in.format, in.layout)) return rc;
  if (const int rc = check_sample_format(who, out.format, out.layout)) return rc;
  if (in.ptr && !in.frames() && in.pitch < in.n) return fail(FSKHIP_E_INVALID, "in_pitch %zu < n_in %zu", in.pitch, in.n);
  if (in.ptr && in.frames() && in.pitch < p->S) return fail(FSKHIP_E_INVALID, "in frame pitch %zu < n_streams %u", in.pitch, p->S);
  if (out.ptr && !out.frames() && out.pitch < out.n) return fail(FSKHIP_E_INVALID, "out_pitch %zu < n_out %zu", out.pitch, out.n);
  if (out.ptr && out.frames() && out.pitch < p->S) return fail(FSKHIP_E_INVALID, "out frame pitch %zu < n_streams %u", out.pitch, p->S);
  if ((reinterpret_cast<uintptr_t>(in.ptr) & (sample_bytes(in.format) - 1u)) != 0) return fail(FSKHIP_E_INVALID, "%s is not aligned to its element size", in_name);
  if ((reinterpret_cast<uintptr_t>(out.ptr) & (sample_bytes(out.format) - 1u)) != 0) return fail(FSKHIP_E_INVALID, "%s is not aligned to its element size", out_name);
  return FSKHIP_OK;
}

// the launches of one quantum, in stream order: ingest, the demodulator's, bookkeeping / TX
int launch_quantum_fmt(fskhip_processor *p, const Side &in, size_t fin_pitch, const Side &out, uint32_t flags, hipStream_t st) {
  if (in.ptr) {
    float *d_x = (float *)const_cast<void *>(in.ptr);
    size_t x_pitch = in.pitch;
    if (!in.floats()) {
      const hipError_t err = launch_ingest(in.ptr, in.format, in.layout, p->S, in.n, in.pitch, p->d_fin, fin_pitch, st);
      if (err == hipErrorInvalidValue) return fail(FSKHIP_E_INVALID, "%u streams x %zu samples are more workgroups than one launch takes", p->S, in.n);
      HIP_TRY(err);
      d_x = p->d_fin; x_pitch = fin_pitch;
    }
    int rc = fskhip_demodulate_device(p->e, d_x, in.n, x_pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, st);
    if (rc != FSKHIP_OK) return rc;
  }
  HIP_TRY(launch_processor_io_fmt(p->e->M, p->e->S.coef, p->T, p->d_bytes, p->bytes_pitch, p->d_counts, in.ptr != nullptr, const_cast<void *>(out.ptr), out.format,
                                  out.layout, out.n, out.pitch, (flags & FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE) != 0, st));
  return FSKHIP_OK;
}

}  // namespace

extern "C" {

int fskhip_processor_process_fmt_device(fskhip_processor *p, const void *d_in, int in_format, int in_layout, size_t n_in, size_t in_pitch, void *d_out,
                                        int out_format, int out_layout, size_t n_out, size_t out_pitch, uint32_t flags, void *hip_stream) {
  const Side in{d_in, in_format, in_layout, n_in, in_pitch}, out{d_out, out_format, out_layout, n_out, out_pitch};
  if (const int rc = fmt_refusal("fskhip_processor_process_fmt_device", p, in, "d_in", out, "d_out")) return rc;
  if (in.floats() && out.floats())
    return fskhip_processor_process_device(p, (float *)const_cast<void *>(d_in), n_in, in_pitch, (float *)d_out, n_out, out_pitch, flags, hip_stream);
  p->used = true;
  if (d_in && !fskhip_demod_supported(p->e)) {
    // let the engine produce its own loud message
    return fskhip_demodulate_device(p->e, (float *)const_cast<void *>(d_in), n_in, in_pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, hip_stream);
  }
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t fin_pitch = n_in ? (n_in + 3) & ~(size_t)3 : 4;   // rows on 16-byte boundaries
  if (d_in) {  // byte slab and float tile of this quantum
    if (const int rc = grow_byte_slab(p, n_in)) return rc;
    if (!in.floats())
      if (const int rc = grow_for_quantum(p, p->d_fin, p->d_fin_cap, fin_pitch * p->S)) return rc;
  }
  return run_quantum_tx(p, !(d_out && n_out) ? kTxNone : out.floats() ? kTxIo : kTxFmt, {(float *)const_cast<void *>(d_in), n_in, in_pitch, (float *)d_out, n_out, out_pitch, flags, st, 0u, in_format, in_layout, out_format, out_layout},
                     d_in != nullptr, [&](uint32_t f) { return launch_quantum_fmt(p, in, fin_pitch, out, f, st); });
}

// Host memory either way.  The samples cross PCIe as they are: a stream-major side as one 2-D copy of its narrow rows (staged rows
// on 16-byte boundaries), a sample-major side as one copy of its n frames -- in at the caller's frame pitch, out packed to n_streams
// elements per frame and spread to the caller's pitch by the copy, whose other columns stay as they are.
int fskhip_processor_process_fmt_host(fskhip_processor *p, const void *in_, int in_format, int in_layout, size_t n_in, size_t in_pitch, void *out_,
                                      int out_format, int out_layout, size_t n_out, size_t out_pitch, uint32_t flags) {
  const Side in{in_, in_format, in_layout, n_in, in_pitch}, out{out_, out_format, out_layout, n_out, out_pitch};
  if (const int rc = fmt_refusal("fskhip_processor_process_fmt_host", p, in, "in", out, "out")) return rc;
  if (in.floats() && out.floats())
    return fskhip_processor_process_host(p, (float *)const_cast<void *>(in_), n_in, in_pitch, (float *)out_, n_out, out_pitch, flags);
  HIP_TRY(hipSetDevice(p->device));
  const size_t S = p->S, isz = sample_bytes(in_format), osz = sample_bytes(out_format);
  const size_t d_in_pitch = in.frames() ? in_pitch : ((n_in * isz + 15) & ~(size_t)15) / isz;
  const size_t in_bytes = in.frames() ? (n_in ? ((n_in - 1) * in_pitch + S) * isz : 0) : S * d_in_pitch * isz;   // (the last frame: its S columns only)
  const EgressStage g = egress_stage(S, n_out, osz, out.frames());
  int rc;
  if (in_ && (rc = grow_for_quantum(p, p->d_nin, p->d_nin_cap, in_bytes ? in_bytes : 16)) != FSKHIP_OK) return rc;
  if (out_ && (rc = grow_for_quantum(p, p->d_nout, p->d_nout_cap, g.bytes ? g.bytes : 16)) != FSKHIP_OK) return rc;
  if (in_ && n_in) {
    if (in.frames()) HIP_TRY(hipMemcpyAsync(p->d_nin, in_, in_bytes, hipMemcpyHostToDevice, p->stream));
    else HIP_TRY(hipMemcpy2DAsync(p->d_nin, d_in_pitch * isz, in_, in_pitch * isz, n_in * isz, S, hipMemcpyHostToDevice, p->stream));
  }
  rc = fskhip_processor_process_fmt_device(p, in_ ? p->d_nin : nullptr, in_format, in_layout, n_in, d_in_pitch ? d_in_pitch : 16 / isz, out_ ? p->d_nout : nullptr,
                                           out_format, out_layout, n_out, g.npitch ? g.npitch : 16 / osz, flags, p->stream);
  if (rc != FSKHIP_OK) return rc;
  if (out_ && n_out) HIP_TRY(hipMemcpy2DAsync(out_, out_pitch * osz, p->d_nout, g.npitch * osz, g.row_bytes, g.rows, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return FSKHIP_OK;
}

}  // extern "C"
