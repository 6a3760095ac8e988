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
  // captured quantum
  hipGraphExec_t graph_exec = nullptr;
  struct Key {
    float *in; size_t n_in, in_pitch; float *out; size_t n_out, out_pitch; uint32_t flags; hipStream_t st; uint32_t ekey;
    bool operator==(const Key &o) const {
      return in == o.in && n_in == o.n_in && in_pitch == o.in_pitch && out == o.out && n_out == o.n_out &&
             out_pitch == o.out_pitch && flags == o.flags && st == o.st && ekey == o.ekey;
    }
  } graph_key{};
};

namespace fsk {

inline void drop_graph(fskhip_processor *p) {
  if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
  p->graph_exec = nullptr;
}

// fsk_processor.hip: the payload store holds rows of at least max_len bytes (a multiple of 64, zero filled), the pending rows
// kept; a captured quantum holds the old pointer and is dropped.  After a device synchronisation.
int processor_grow_payload(fskhip_processor *p, size_t max_len);

}  // namespace fsk
