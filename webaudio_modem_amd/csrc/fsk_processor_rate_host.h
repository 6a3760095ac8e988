// fsk_processor_rate_host.h -- what the two FSKProcessor quanta at an outer rate share (fsk_processor_rate.hip: through two
// fskhip_resampler handles; fsk_processor_ratecvt.hip: through two fskhip_ratecvt handles), each piece once: a side of the call,
// what both forms refuse before any device call, and the _host form's staging round the unit's own device quantum.  The handles
// are taken by their common base (RateHost, fsk_filter_host.h); how a unit names them is its HandleWords.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "fsk_engine.h"
#include "fsk_filter_host.h"
#include "fsk_launch.h"
#include "fsk_plan.h"
#include "fsk_proc.h"

namespace fsk {

struct Side {
  const void *ptr; int format, layout; size_t n, pitch; RateHost *r;
  bool frames() const { return layout == FSKHIP_LAYOUT_SAMPLE_MAJOR; }
};

// a unit's words for its handles: the two directions' names, by the direction's number, and what a handle of the other one does
// ("the up handle resamples down", "the capture handle converts for playback")
struct HandleWords { const char *name[2]; const char *verb; };

// a side's handle: there, of the side's direction, and the processor's in streams and device
inline int handle_refusal(const char *who, const HandleWords &W, const fskhip_processor *p, const RateHost *r, int direction) {
  const char *const name = W.name[direction];
  if (!r) return fail(FSKHIP_E_INVALID, "%s: null %s handle", who, name);
  if (r->direction != direction) return fail(FSKHIP_E_INVALID, "%s: the %s handle %s %s", who, name, W.verb, W.name[r->direction]);
  if (r->S != p->S) return fail(FSKHIP_E_INVALID, "%s: the %s handle has %u streams, the processor %u", who, name, r->S, p->S);
  if (r->device != p->device) return fail(FSKHIP_E_INVALID, "%s: the %s handle is on device %d, the processor on %d", who, name, r->device, p->device);
  return FSKHIP_OK;
}

// what both forms refuse before any device call, in the header's order; the input side's handle is of direction 0, the output
// side's of direction 1; in_name / out_name: the arguments as the form calls them
inline int rate_refusal(const char *who, const HandleWords &W, const fskhip_processor *p, const Side &in, const char *in_name, const Side &out, const char *out_name) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (const int rc = check_sample_format(who, in.format, in.layout)) return rc;
  if (const int rc = check_sample_format(who, out.format, out.layout)) return rc;
  if (in.ptr)
    if (const int rc = handle_refusal(who, W, p, in.r, 0)) return rc;
  if (out.ptr)
    if (const int rc = handle_refusal(who, W, p, out.r, 1)) return rc;
  if (in.ptr && !in.frames() && in.pitch < in.n) return fail(FSKHIP_E_INVALID, "in_pitch %zu < n_in %zu", in.pitch, in.n);
  if (in.ptr && in.frames() && in.pitch < p->S) return fail(FSKHIP_E_INVALID, "in frame pitch %zu < n_streams %u", in.pitch, p->S);
  if (out.ptr && !out.frames() && out.pitch < out.n) return fail(FSKHIP_E_INVALID, "out_pitch %zu < n_out %zu", out.pitch, out.n);
  if (out.ptr && out.frames() && out.pitch < p->S) return fail(FSKHIP_E_INVALID, "out frame pitch %zu < n_streams %u", out.pitch, p->S);
  if ((reinterpret_cast<uintptr_t>(in.ptr) & (sample_bytes(in.format) - 1u)) != 0) return fail(FSKHIP_E_INVALID, "%s is not aligned to its element size", in_name);
  if ((reinterpret_cast<uintptr_t>(out.ptr) & (sample_bytes(out.format) - 1u)) != 0) return fail(FSKHIP_E_INVALID, "%s is not aligned to its element size", out_name);
  return FSKHIP_OK;
}

inline int launch_failed(const char *who, hipError_t err, uint32_t n_streams, size_t n) {
  if (err == hipErrorInvalidValue) return fail(FSKHIP_E_INVALID, "%s: %u streams x %zu samples are more workgroups than one launch takes", who, n_streams, n);
  HIP_TRY(err);
  return FSKHIP_OK;
}

// The _host form behind its refusals, host memory either way: the outer rate samples cross PCIe as they are, staged as
// fskhip_processor_process_fmt_host stages its own, round device(in, out) -- the unit's quantum on the staged sides, on the
// processor's stream.  Synchronous.
template <class Device>
int rate_host_quantum(fskhip_processor *p, const Side &in, const Side &out, Device device) {
  HIP_TRY(hipSetDevice(p->device));
  const size_t S = p->S, isz = sample_bytes(in.format), osz = sample_bytes(out.format);
  const size_t d_in_pitch = in.frames() ? in.pitch : ((in.n * isz + 15) & ~(size_t)15) / isz;
  const size_t in_bytes = in.frames() ? (in.n ? ((in.n - 1) * in.pitch + S) * isz : 0) : S * d_in_pitch * isz;   // (the last frame: its S columns only)
  const EgressStage g = egress_stage(S, out.n, osz, out.frames());
  int rc;
  if (in.ptr && (rc = grow_for_quantum(p, p->d_nin, p->d_nin_cap, in_bytes ? in_bytes : 16)) != FSKHIP_OK) return rc;
  if (out.ptr && (rc = grow_for_quantum(p, p->d_nout, p->d_nout_cap, g.bytes ? g.bytes : 16)) != FSKHIP_OK) return rc;
  if (in.ptr && in.n) {
    if (in.frames()) HIP_TRY(hipMemcpyAsync(p->d_nin, in.ptr, in_bytes, hipMemcpyHostToDevice, p->stream));
    else HIP_TRY(hipMemcpy2DAsync(p->d_nin, d_in_pitch * isz, in.ptr, in.pitch * isz, in.n * isz, S, hipMemcpyHostToDevice, p->stream));
  }
  const Side d_in{in.ptr ? p->d_nin : nullptr, in.format, in.layout, in.n, d_in_pitch ? d_in_pitch : 16 / isz, in.r};
  const Side d_out{out.ptr ? p->d_nout : nullptr, out.format, out.layout, out.n, g.npitch ? g.npitch : 16 / osz, out.r};
  if ((rc = device(d_in, d_out)) != FSKHIP_OK) return rc;
  if (out.ptr && out.n)
    HIP_TRY(hipMemcpy2DAsync(const_cast<void *>(out.ptr), out.pitch * osz, p->d_nout, g.npitch * osz, g.row_bytes, g.rows, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return FSKHIP_OK;
}

}  // namespace fsk
