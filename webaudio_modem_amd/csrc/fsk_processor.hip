// fsk_processor.hip -- C ABI of the FSKProcessor / ChunkedModulator streaming contract (include/fskhip_next.h,
// SURVEY.md 8(f1)): per-stream RX byte ring and pending modulation resident on the device, one process() per
// quantum = the demodulator launch(es) + one bookkeeping/TX launch, optionally replayed as a captured hipGraph
// (a 128-sample quantum is launch-bound, not bandwidth-bound).
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fsk_engine.h"
#include "fsk_launch.h"
#include "fsk_proc.h"

using namespace fsk;

namespace {

// the launches of one quantum, in stream order
int launch_quantum(fskhip_processor *p, float *d_in, size_t n_in, size_t in_pitch, float *d_out, size_t n_out,
                   size_t out_pitch, uint32_t flags, hipStream_t st) {
  if (d_in) {
    int rc = fskhip_demodulate_device(p->e, d_in, n_in, in_pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, st);
    if (rc != FSKHIP_OK) return rc;
  }
  HIP_TRY(launch_processor_io(p->e->M, p->e->S.coef, p->T, p->d_bytes, p->bytes_pitch, p->d_counts,
                              d_in != nullptr, d_out, n_out, out_pitch, (flags & FSKHIP_PROC_CLEAR_RX_ON_TX_COMPLETE) != 0, st));
  return FSKHIP_OK;
}

}  // namespace

namespace fsk {
int processor_grow_payload(fskhip_processor *p, size_t max_len) {
  if (max_len <= p->T.tx_payload_pitch) return FSKHIP_OK;
  const size_t S = p->S;
  const size_t np = (max_len + 63) & ~(size_t)63;
  uint8_t *nbuf = nullptr;
  int rc = dev_alloc(nbuf, np * S);
  if (rc != FSKHIP_OK) return rc;
  HIP_TRY(hipMemset(nbuf, 0, np * S));
  if (p->T.tx_payload) {
    HIP_TRY(hipMemcpy2D(nbuf, np, p->T.tx_payload, p->T.tx_payload_pitch, p->T.tx_payload_pitch, S, hipMemcpyDeviceToDevice));
    (void)hipFree(p->T.tx_payload);
  }
  p->T.tx_payload = nbuf;
  p->T.tx_payload_pitch = np;
  drop_graph(p);  // the captured launch holds the old pointer
  return FSKHIP_OK;
}
}  // namespace fsk

extern "C" {

int fskhip_processor_destroy(fskhip_processor *p) {
  if (!p) return FSKHIP_OK;
  (void)hipSetDevice(p->device);
  (void)hipDeviceSynchronize();
  drop_graph(p);
  void *bufs[] = {p->T.rx_buf, p->T.rx_w, p->T.rx_r, p->T.rx_len, p->T.tx_payload, p->T.tx_phase, p->T.tx_pos, p->T.tx_len,
                  p->T.tx_in_bit, p->T.tx_bit_idx, p->T.tx_cur_bit, p->T.tx_n_payload, p->T.tx_pending, p->T.tx_completed,
                  p->d_bytes, p->d_counts, p->d_eod, p->d_in, p->d_out, p->d_stage, p->d_u32, p->d_mask, p->d_lists, p->d_fin, p->d_ftx, p->d_nin, p->d_nout};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
  return FSKHIP_OK;
}

int fskhip_processor_create(fskhip_engine *e, uint32_t rx_capacity, fskhip_processor **out) {
  if (!e || !out) return fail(FSKHIP_E_INVALID, "fskhip_processor_create: null argument");
  if (rx_capacity == 0) return fail(FSKHIP_E_INVALID, "rx_capacity must be > 0");
  fskhip_processor *p = new (std::nothrow) fskhip_processor();
  if (!p) return fail(FSKHIP_E_NOMEM, "out of host memory");
  p->e = e; p->device = e->device; p->S = fskhip_n_streams(e);
  const size_t S = p->S;
  ProcState &T = p->T;
  T.rx_cap = rx_capacity;
  int rc = FSKHIP_OK;
  hipError_t herr = hipSetDevice(p->device);
  if (herr != hipSuccess) { delete p; return fail(FSKHIP_E_HIP, "hipSetDevice: %s", hipGetErrorString(herr)); }
#define PROC_TRY(expr)                                   \
  do {                                                   \
    if (rc == FSKHIP_OK) rc = (expr);                    \
  } while (0)
  PROC_TRY(dev_alloc(T.rx_buf, S * rx_capacity));
  PROC_TRY(dev_alloc(T.rx_w, S)); PROC_TRY(dev_alloc(T.rx_r, S)); PROC_TRY(dev_alloc(T.rx_len, S));
  PROC_TRY(dev_alloc(T.tx_phase, S));
  PROC_TRY(dev_alloc(T.tx_pos, S)); PROC_TRY(dev_alloc(T.tx_len, S)); PROC_TRY(dev_alloc(T.tx_in_bit, S));
  PROC_TRY(dev_alloc(T.tx_bit_idx, S)); PROC_TRY(dev_alloc(T.tx_cur_bit, S)); PROC_TRY(dev_alloc(T.tx_n_payload, S));
  PROC_TRY(dev_alloc(T.tx_pending, S)); PROC_TRY(dev_alloc(T.tx_completed, S));
  PROC_TRY(dev_alloc(p->d_counts, S)); PROC_TRY(dev_alloc(p->d_eod, S)); PROC_TRY(dev_alloc(p->d_u32, 4 * S + 4));
  PROC_TRY(dev_alloc(p->d_mask, S));
#undef PROC_TRY
  if (rc == FSKHIP_OK) {
    uint32_t *zero[] = {T.rx_w, T.rx_r, T.rx_len, T.tx_pos, T.tx_len, T.tx_in_bit, T.tx_bit_idx, T.tx_cur_bit,
                        T.tx_n_payload, T.tx_pending, T.tx_completed, p->d_counts, p->d_eod};
    for (uint32_t *z : zero)
      if (hipMemset(z, 0, sizeof(uint32_t) * S) != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipMemset failed");
    if (hipMemset(T.tx_phase, 0, sizeof(double) * S) != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipMemset failed");
    if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipStreamCreate failed");
    if (hipDeviceSynchronize() != hipSuccess) rc = fail(FSKHIP_E_HIP, "hipDeviceSynchronize failed");
  }
  if (rc != FSKHIP_OK) {
    std::string keep = fskhip_last_error();
    fskhip_processor_destroy(p);
    return fail(rc, "%s", keep.c_str());
  }
  *out = p;
  return FSKHIP_OK;
}

int fskhip_processor_process_device(fskhip_processor *p, float *d_in, size_t n_in, size_t in_pitch, float *d_out,
                                    size_t n_out, size_t out_pitch, uint32_t flags, void *hip_stream) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (d_in && in_pitch < n_in) return fail(FSKHIP_E_INVALID, "in_pitch %zu < n_in %zu", in_pitch, n_in);
  if (d_out && out_pitch < n_out) return fail(FSKHIP_E_INVALID, "out_pitch %zu < n_out %zu", out_pitch, n_out);
  p->used = true;
  if (d_in && !fskhip_demod_supported(p->e)) {
    // let the engine produce its own loud message
    return fskhip_demodulate_device(p->e, d_in, n_in, in_pitch, p->d_bytes, p->bytes_pitch, p->d_counts, p->d_eod, 0u, hip_stream);
  }
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  if (d_in)   // byte slab of this quantum
    if (const int rc = grow_byte_slab(p, n_in)) return rc;
  return run_quantum_tx(p, d_out && n_out ? kTxIo : kTxNone, {d_in, n_in, in_pitch, d_out, n_out, out_pitch, flags, st, 0u}, d_in != nullptr,
                     [&](uint32_t f) { return launch_quantum(p, d_in, n_in, in_pitch, d_out, n_out, out_pitch, f, st); });
}

int fskhip_processor_process_host(fskhip_processor *p, float *in, size_t n_in, size_t in_pitch, float *out, size_t n_out,
                                  size_t out_pitch, uint32_t flags) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (in && in_pitch < n_in) return fail(FSKHIP_E_INVALID, "in_pitch %zu < n_in %zu", in_pitch, n_in);
  if (out && out_pitch < n_out) return fail(FSKHIP_E_INVALID, "out_pitch %zu < n_out %zu", out_pitch, n_out);
  HIP_TRY(hipSetDevice(p->device));
  const size_t S = p->S;
  const size_t ip = (n_in + 3) & ~(size_t)3, op = (n_out + 3) & ~(size_t)3;
  int rc;
  if (in && (rc = ensure(p->d_in, p->d_in_cap, (ip ? ip : 4) * S)) != FSKHIP_OK) return rc;
  if (out && (rc = ensure(p->d_out, p->d_out_cap, (op ? op : 4) * S)) != FSKHIP_OK) return rc;
  if (in && n_in)
    HIP_TRY(hipMemcpy2DAsync(p->d_in, ip * sizeof(float), in, in_pitch * sizeof(float), n_in * sizeof(float), S,
                             hipMemcpyHostToDevice, p->stream));
  rc = fskhip_processor_process_device(p, in ? p->d_in : nullptr, n_in, ip ? ip : 4, out ? p->d_out : nullptr, n_out,
                                       op ? op : 4, flags, p->stream);
  if (rc != FSKHIP_OK) return rc;
  if (out && n_out)
    HIP_TRY(hipMemcpy2DAsync(out, out_pitch * sizeof(float), p->d_out, op * sizeof(float), n_out * sizeof(float), S,
                             hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return FSKHIP_OK;
}

const char *fskhip_processor_last_tx_kernel(const fskhip_processor *p) { return p ? p->last_tx_kernel : ""; }

int fskhip_processor_graph_stats(const fskhip_processor *p, uint64_t *captures, uint64_t *replays) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (captures) *captures = p->graph_captures;
  if (replays) *replays = p->graph_replays;
  return FSKHIP_OK;
}

int fskhip_processor_modulate_host(fskhip_processor *p, const uint8_t *payloads, const uint32_t *lens, size_t payload_pitch,
                                   const uint8_t *mask) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (!lens) return fail(FSKHIP_E_INVALID, "null lens");
  p->used = true;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t S = p->S;
  std::vector<uint32_t> pending(S);
  HIP_TRY(hipMemcpy(pending.data(), p->T.tx_pending, sizeof(uint32_t) * S, hipMemcpyDeviceToHost));
  size_t max_len = 0;
  for (size_t s = 0; s < S; s++) {
    if (mask && !mask[s]) continue;
    if (pending[s]) return fail(FSKHIP_E_BUSY, "Modulation already in progress (stream %zu)", s);
    if (lens[s] > payload_pitch) return fail(FSKHIP_E_INVALID, "lens[%zu] = %u exceeds payload_pitch %zu", s, lens[s], payload_pitch);
    if (lens[s] && !payloads) return fail(FSKHIP_E_INVALID, "null payloads");
    if (lens[s] > max_len) max_len = lens[s];
  }
  if (const int grc = processor_grow_payload(p, max_len)) return grc;
  int rc;
  if ((rc = ensure(p->d_stage, p->d_stage_cap, (payload_pitch ? payload_pitch : 1) * S)) != FSKHIP_OK) return rc;
  if (payload_pitch && payloads) HIP_TRY(hipMemcpy(p->d_stage, payloads, payload_pitch * S, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_u32, lens, sizeof(uint32_t) * S, hipMemcpyHostToDevice));
  if (mask) HIP_TRY(hipMemcpy(p->d_mask, mask, S, hipMemcpyHostToDevice));
  HIP_TRY(launch_processor_tx_start(p->e->M, p->T, p->d_stage, p->d_u32, payload_pitch,
                                    mask ? p->d_mask : nullptr, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

int fskhip_processor_tx_state_host(fskhip_processor *p, uint32_t *pos, uint32_t *total, uint8_t *pending, uint32_t *completed) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t S = p->S;
  if (pos) HIP_TRY(hipMemcpy(pos, p->T.tx_pos, sizeof(uint32_t) * S, hipMemcpyDeviceToHost));
  if (total) HIP_TRY(hipMemcpy(total, p->T.tx_len, sizeof(uint32_t) * S, hipMemcpyDeviceToHost));
  if (completed) HIP_TRY(hipMemcpy(completed, p->T.tx_completed, sizeof(uint32_t) * S, hipMemcpyDeviceToHost));
  if (pending) {
    std::vector<uint32_t> tmp(S);
    HIP_TRY(hipMemcpy(tmp.data(), p->T.tx_pending, sizeof(uint32_t) * S, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < S; s++) pending[s] = tmp[s] ? 1 : 0;
  }
  return FSKHIP_OK;
}

int fskhip_processor_rx_drain_host(fskhip_processor *p, uint8_t *out, size_t out_pitch, uint32_t *counts) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (!counts || (out_pitch && !out)) return fail(FSKHIP_E_INVALID, "null buffer");
  p->used = true;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t S = p->S;
  int rc;
  if ((rc = ensure(p->d_stage, p->d_stage_cap, (out_pitch ? out_pitch : 1) * S)) != FSKHIP_OK) return rc;
  HIP_TRY(launch_processor_rx_drain(p->T, p->S, p->d_stage, out_pitch, p->d_u32, nullptr));
  HIP_TRY(hipMemcpy(counts, p->d_u32, sizeof(uint32_t) * S, hipMemcpyDeviceToHost));
  if (out_pitch) HIP_TRY(hipMemcpy(out, p->d_stage, out_pitch * S, hipMemcpyDeviceToHost));
  for (size_t s = 0; s < S; s++)
    if (counts[s] > out_pitch) return fail(FSKHIP_E_OVERFLOW, "stream %zu held %u bytes, slab holds %zu", s, counts[s], out_pitch);
  return FSKHIP_OK;
}

// what both forms of the sparse drain refuse before they touch the device, in the header's order
static int sparse_drain_refusal(const char *fn, const fskhip_processor *p, const void *totals, const char *totals_name, const void *streams,
                                const void *offsets, uint32_t cap_streams, const void *data, size_t cap_bytes) {
  if (!totals) return fail(FSKHIP_E_INVALID, "%s: null %s", fn, totals_name);
  if (cap_streams && (!streams || !offsets)) return fail(FSKHIP_E_INVALID, "%s: null streams or offsets with cap_streams %u", fn, cap_streams);
  if (cap_bytes && !data) return fail(FSKHIP_E_INVALID, "%s: null data with cap_bytes %zu", fn, cap_bytes);
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if ((uint64_t)p->S * p->T.rx_cap > 0xFFFFFFFFull)
    return fail(FSKHIP_E_UNSUPPORTED, "%s: %u streams x rx_capacity %u exceed the 32-bit offsets", fn, p->S, p->T.rx_cap);
  return FSKHIP_OK;
}

int fskhip_processor_rx_drain_sparse_host(fskhip_processor *p, const uint8_t *mask, uint32_t min_len, uint32_t *streams,
                                          uint32_t *offsets, uint32_t cap_streams, uint8_t *data, size_t cap_bytes,
                                          uint32_t *n_active, uint32_t *n_bytes) {
  static const char fn[] = "fskhip_processor_rx_drain_sparse_host";
  if (const int rc = sparse_drain_refusal(fn, p, n_active && n_bytes ? (const void *)n_active : nullptr, "n_active or n_bytes", streams, offsets,
                                          cap_streams, data, cap_bytes))
    return rc;
  p->used = true;
  *n_active = 0u; *n_bytes = 0u;
  const size_t S = p->S;
  if (S == 0) {
    if (offsets) offsets[0] = 0u;
    return FSKHIP_OK;
  }
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  if (mask) HIP_TRY(hipMemcpy(p->d_mask, mask, S, hipMemcpyHostToDevice));
  const uint8_t *d_mask = mask ? p->d_mask : nullptr;
  uint32_t *d_totals = p->d_u32 + 4 * S;
  HIP_TRY(launch_drain_sparse_size(p->T, p->S, d_mask, min_len, cap_streams, cap_bytes, p->d_u32, d_totals, nullptr));
  uint32_t totals[2] = {0u, 0u};
  HIP_TRY(hipMemcpy(totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost));
  *n_active = totals[0]; *n_bytes = totals[1];
  if (totals[0] > cap_streams || totals[1] > cap_bytes)
    return fail(FSKHIP_E_OVERFLOW, "%u streams hold %u bytes, the lists hold %u streams and %zu bytes (nothing was drained)", totals[0], totals[1],
                cap_streams, cap_bytes);
  if (totals[0] == 0u) {   // nothing selected: nothing to pack
    if (offsets) offsets[0] = 0u;
    return FSKHIP_OK;
  }
  int rc;   // staging for what is there, not for n_streams x rx_capacity
  if ((rc = ensure(p->d_stage, p->d_stage_cap, (size_t)totals[1])) != FSKHIP_OK) return rc;
  if ((rc = ensure(p->d_lists, p->d_lists_cap, 2 * (size_t)totals[0] + 1)) != FSKHIP_OK) return rc;
  uint32_t *d_streams = p->d_lists, *d_offsets = p->d_lists + totals[0];
  HIP_TRY(launch_drain_sparse_pack(p->T, p->S, d_mask, min_len, p->d_u32, d_totals, d_streams, d_offsets, p->d_stage, nullptr));
  HIP_TRY(hipMemcpy(streams, d_streams, sizeof(uint32_t) * totals[0], hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(offsets, d_offsets, sizeof(uint32_t) * ((size_t)totals[0] + 1), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(data, p->d_stage, totals[1], hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}

int fskhip_processor_rx_drain_sparse_device(fskhip_processor *p, const uint8_t *d_mask, uint32_t min_len, uint32_t *d_streams,
                                            uint32_t *d_offsets, uint32_t cap_streams, uint8_t *d_data, size_t cap_bytes,
                                            uint32_t *d_totals, void *hip_stream) {
  if (const int rc = sparse_drain_refusal("fskhip_processor_rx_drain_sparse_device", p, d_totals, "d_totals", d_streams, d_offsets, cap_streams, d_data,
                                          cap_bytes))
    return rc;
  p->used = true;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(launch_drain_sparse_size(p->T, p->S, d_mask, min_len, cap_streams, cap_bytes, p->d_u32, d_totals, st));
  HIP_TRY(launch_drain_sparse_pack(p->T, p->S, d_mask, min_len, p->d_u32, d_totals, d_streams, d_offsets, d_data, st));
  return FSKHIP_OK;
}

int fskhip_processor_rx_length_host(fskhip_processor *p, uint32_t *lengths) {
  if (!p || !lengths) return fail(FSKHIP_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(lengths, p->T.rx_len, sizeof(uint32_t) * p->S, hipMemcpyDeviceToHost));
  return FSKHIP_OK;
}

int fskhip_processor_reset(fskhip_processor *p, int64_t stream) {
  if (!p) return fail(FSKHIP_E_INVALID, "null processor");
  if (stream >= (int64_t)p->S) return fail(FSKHIP_E_INVALID, "stream out of range");
  p->used = true;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(launch_processor_reset(p->T, p->S, stream, true, true, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return FSKHIP_OK;
}

}  // extern "C"
