// fsk_proc.h -- struct fskhip_processor and what the two C-ABI units over it share (fsk_processor.hip: the streaming contract;
// fsk_processor_remap_api.hip: remap, snapshot, restore); its buffers come from fsk_host.h's dev_alloc.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "fsk_engine.h"

struct fskhip_processor {
  fskhip_engine *e = nullptr;
  int device = 0;
  uint32_t S = 0;
  fsk::ProcState T{};
  bool used = false;   // a process, modulate, drain or reset call has been made: no longer what fskhip_processor_create left
  const char *last_tx_kernel = "";   // fskhip_processor_last_tx_kernel: what the last quantum's TX side ran (fsk::kTx* below)
  // demodulator outputs of the current quantum
  uint8_t *d_bytes = nullptr; size_t bytes_pitch = 0;
  uint32_t *d_counts = nullptr, *d_eod = nullptr;
  // staging for the _host entry points
  hipStream_t stream = nullptr;
  float *d_in = nullptr; size_t d_in_cap = 0;
  float *d_out = nullptr; size_t d_out_cap = 0;
  uint8_t *d_stage = nullptr; size_t d_stage_cap = 0;
  uint32_t *d_u32 = nullptr;   // [4][S] + 4 words of scratch (the 4: the sparse drain's totals behind its workgroup pairs)
  uint32_t *d_lists = nullptr; size_t d_lists_cap = 0;   // the sparse drain's streams[] and offsets[] on their way to the host
  uint8_t *d_mask = nullptr;
  // fskhip_processor_process_fmt_*: the float tile [S][fin_pitch] the ingest kernel widens a quantum into (rows on 16-byte
  // boundaries; grown outside any capture), and the _host form's samples as they cross PCIe, either way
  float *d_fin = nullptr; size_t d_fin_cap = 0;
  // fskhip_processor_process_rate_*: the float tile [S][pitch] of a quantum whose decimator the fused kernel does not take (grown
  // outside any capture)
  float *d_ftx = nullptr; size_t d_ftx_cap = 0;
  uint8_t *d_nin = nullptr; size_t d_nin_cap = 0;
  uint8_t *d_nout = nullptr; size_t d_nout_cap = 0;
  // captured quantum
  hipGraphExec_t graph_exec = nullptr;
  uint64_t graph_captures = 0, graph_replays = 0;   // fskhip_processor_graph_stats: quanta captured afresh / replayed from the last capture
  struct Key {
    float *in; size_t n_in, in_pitch; float *out; size_t n_out, out_pitch; uint32_t flags; hipStream_t st; uint32_t ekey;
    int in_format = FSKHIP_SAMPLES_F32, in_layout = FSKHIP_LAYOUT_STREAM_MAJOR, out_format = FSKHIP_SAMPLES_F32, out_layout = FSKHIP_LAYOUT_STREAM_MAJOR;
    bool operator==(const Key &o) const {
      return in == o.in && n_in == o.n_in && in_pitch == o.in_pitch && out == o.out && n_out == o.n_out &&
             out_pitch == o.out_pitch && flags == o.flags && st == o.st && ekey == o.ekey && in_format == o.in_format &&
             in_layout == o.in_layout && out_format == o.out_format && out_layout == o.out_layout;
    }
  } graph_key{};
};

namespace fsk {

// What fskhip_processor_last_tx_kernel reports: the kernel of a quantum's TX side, or the two launches that stand for one.  Every
// process form decides it in front of its quantum and sets it behind one that was issued (run_quantum_tx): launched, captured or
// replayed.
constexpr const char *kTxNone = "";
constexpr const char *kTxIo = "processor_io_kernel";
constexpr const char *kTxFmt = "processor_io_fmt_kernel";
constexpr const char *kTxRate = "processor_io_rate_kernel";
constexpr const char *kTxRatePair = "processor_io_kernel+resample_down_kernel";
constexpr const char *kTxRatecvt = "processor_io_ratecvt_kernel";
constexpr const char *kTxRatecvtAny = "processor_io_ratecvt_kernel<any>";
constexpr const char *kTxRatecvtPair = "processor_io_kernel+ratecvt_playback_kernel";
constexpr const char *kTxRatecvtAnyPair = "processor_io_kernel+ratecvt_playback_any_kernel";

inline void drop_graph(fskhip_processor *p) {
  if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
  p->graph_exec = nullptr;
}

// One quantum of fskhip_processor_process_device / _process_fmt_device behind their argument checks and buffer growth: launch(flags)
// issues the quantum's launches on key.st, in stream order.  Plainly; or, with FSKHIP_PROC_GRAPH, captured once as one linear graph
// on the caller's stream and replayed while the key -- the call's arguments as the caller filled them in, with the flags and the
// engine's launch key as they are taken here -- stays the same.  has_in: the call demodulates n_in samples (a replay's host-side
// accounting).
template <typename Launch>
int run_quantum(fskhip_processor *p, fskhip_processor::Key key, bool has_in, Launch launch) {
  // timing events / the trace capture are per-launch host decisions: no replay while either is armed
  engine_refresh_kernel_choice(p->e);
  if (engine_launch_key(p->e) & (8u | 16u)) key.flags &= ~FSKHIP_PROC_GRAPH;
  if (!(key.flags & FSKHIP_PROC_GRAPH)) return launch(key.flags);

  if (!key.st) return fail(FSKHIP_E_INVALID, "FSKHIP_PROC_GRAPH needs an explicit stream (the null stream cannot be captured)");
  key.ekey = engine_launch_key(p->e);
  if (!p->graph_exec || !(key == p->graph_key)) {
    drop_graph(p);
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(key.st, hipStreamCaptureModeThreadLocal));
    int rc = launch(key.flags);
    hipError_t cerr = hipStreamEndCapture(key.st, &graph);
    if (rc != FSKHIP_OK) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    if (cerr != hipSuccess) return fail(FSKHIP_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(cerr));
    hipError_t ierr = hipGraphInstantiate(&p->graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ierr != hipSuccess) { p->graph_exec = nullptr; return fail(FSKHIP_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ierr)); }
    p->graph_key = key;
    p->graph_captures++;
    // the capture itself already did the host-side accounting of one call; it launched nothing
    HIP_TRY(hipGraphLaunch(p->graph_exec, key.st));
    return FSKHIP_OK;
  }
  if (has_in) engine_note_replayed_call(p->e, key.n_in);
  HIP_TRY(hipGraphLaunch(p->graph_exec, key.st));
  p->graph_replays++;
  return FSKHIP_OK;
}

// run_quantum, and behind a quantum that was issued the name of its TX path (fskhip_processor_last_tx_kernel): a call that fails
// here or in a launch leaves the name of the quantum before, as a refused one does
template <typename Launch>
int run_quantum_tx(fskhip_processor *p, const char *tx, fskhip_processor::Key key, bool has_in, Launch launch) {
  const int rc = run_quantum(p, key, has_in, launch);
  if (rc == FSKHIP_OK) p->last_tx_kernel = tx;
  return rc;
}

// the demodulators' byte slab [S][bytes_pitch] holds a quantum of n_in samples: grown outside any capture, and a captured quantum,
// which holds the old pointer, is dropped
inline int grow_byte_slab(fskhip_processor *p, size_t n_in) {
  const size_t need = engine_max_bytes(p->e, n_in);
  if (need <= p->bytes_pitch) return FSKHIP_OK;
  HIP_TRY(hipDeviceSynchronize());
  drop_graph(p);
  if (p->d_bytes) (void)hipFree(p->d_bytes);
  p->d_bytes = nullptr; p->bytes_pitch = 0;
  int rc = dev_alloc(p->d_bytes, need * p->S);
  if (rc != FSKHIP_OK) return rc;
  p->bytes_pitch = need;
  return FSKHIP_OK;
}

// a device buffer that only grows, outside any capture: the captured quantum holds the old pointer and is dropped
template <typename T>
int grow_for_quantum(fskhip_processor *p, T *&buf, size_t &cap, size_t need) {
  if (need <= cap) return FSKHIP_OK;
  HIP_TRY(hipDeviceSynchronize());
  drop_graph(p);
  return ensure(buf, cap, need);
}

// fsk_processor.hip: the payload store holds rows of at least max_len bytes (a multiple of 64, zero filled), the pending rows
// kept; a captured quantum holds the old pointer and is dropped.  After a device synchronisation.
int processor_grow_payload(fskhip_processor *p, size_t max_len);

}  // namespace fsk
