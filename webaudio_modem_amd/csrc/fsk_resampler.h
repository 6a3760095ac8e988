// fsk_resampler.h -- struct fskhip_resampler, for the C-ABI units over it (fsk_resample.hip: the handle and its own calls;
// fsk_processor_rate.hip: the FSKProcessor quantum at the low rate, which runs a handle's filter inside its own launches;
// fsk_resample_remap_api.hip: remap, snapshot and restore).  Not part of the ABI.
#pragma once
#include <vector>

#include "fsk_filter_host.h"

struct fskhip_resampler : fsk::FilterHost {
  int direction = 0;
  uint32_t L = 1, n_taps = 0, H = 0;      // H: floats of history per stream (resample_history)
  double *d_taps = nullptr;               // fp64 path: as given (down), phase by phase [L][K] (up)
  float *d_taps32 = nullptr;              // the same, rounded once on the host (fp32 path)
  float *hist[2] = {nullptr, nullptr};    // ping-pong: [cur] is read by the next call
  int cur = 0;
  uint32_t *d_lens = nullptr;             // the _host form's per-stream lengths
  std::vector<double> h_taps;             // the taps as given to create: what a remap designs its new handle from and a snapshot carries

  const void *taps() const { return precision == FSKHIP_PRECISION_F64 ? (const void *)d_taps : (const void *)d_taps32; }
};
