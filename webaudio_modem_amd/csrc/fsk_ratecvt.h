// fsk_ratecvt.h -- struct fskhip_ratecvt, for the C-ABI units over it (fsk_ratecvt.hip: the handle and its own calls;
// fsk_processor_ratecvt.hip: the FSKProcessor quantum at the converter's outer rate, which runs a handle's filter inside its own
// launches; fsk_ratecvt_remap_api.hip: remap, snapshot and restore).  Not part of the ABI.
#pragma once
#include <vector>

#include "fsk_filter_host.h"

struct fskhip_ratecvt : fsk::RateHost {   // L: the up factor; H: resample_history(0, L, n_taps); the taps [K][L] in output order (fsk_ratecvt_plan.h)
  uint32_t M = 1;                          // the down factor
  uint32_t *d_table = nullptr;             // [L]: ratecvt_table_word
  uint32_t pos = 0;                        // inputs taken since the last period boundary, < M: all streams' (fsk_ratecvt_plan.h)
  std::vector<double> h_taps;              // the taps as given to create: what a remap designs its new handle from and a snapshot carries
};
