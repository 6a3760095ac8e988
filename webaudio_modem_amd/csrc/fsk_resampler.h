// fsk_resampler.h -- struct fskhip_resampler, for the C-ABI units over it (fsk_resample.hip: the handle and its own calls;
// fsk_processor_rate.hip: the FSKProcessor quantum at the low rate, which runs a handle's filter inside its own launches;
// fsk_resample_remap_api.hip: remap, snapshot and restore).  Not part of the ABI.
#pragma once
#include <vector>

#include "fsk_filter_host.h"

struct fskhip_resampler : fsk::RateHost {   // L: the factor; H: resample_history; the taps as given (down), phase by phase [L][K] (up)
  std::vector<double> h_taps;               // the taps as given to create: what a remap designs its new handle from and a snapshot carries
};
