// fsk_xmodem_handles.h -- the three resident XModem handles (fskhip_xmodem_rx / _tx / _recv) as their own C-ABI units
// (fsk_xmodem_rx_api.hip, fsk_xmodem_tx_api.hip, fsk_xmodem_recv_api.hip) and the unit that carries them through remap, snapshot and
// restore (fsk_xmodem_remap_api.hip) share them.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "fsk_launch.h"
#include "fsk_proc.h"

namespace fsk {
// fsk_xmodem_timer_api.hip: a file receiver or a sender is going away -- the wait timers created over it refuse every call from now on
void xmodem_timers_orphan(const void *handle);
}  // namespace fsk

using fsk::XmRxState; using fsk::XmRxScratch; using fsk::XmTxState; using fsk::XmTxScratch; using fsk::XmRecvState; using fsk::XmRecvScratch;

struct fskhip_xmodem_rx {
  fskhip_processor *p = nullptr;
  int device = 0;   // the processor's, kept here: destroy does not read the processor, which may be gone by then
  bool used = false;   // a poll, reset or state_set call has been made: no longer what create left (a remap or restore wants a fresh destination)
  XmRxState X{};
  XmRxScratch W{};
  uint32_t *d_totals = nullptr;
  // staging for the _host form
  uint8_t *d_mask = nullptr;
  uint32_t *d_lists = nullptr; size_t d_lists_cap = 0;            // streams[] and offsets[]
  fskhip_xmodem_result *d_results = nullptr; size_t d_results_cap = 0;
  uint8_t *d_data = nullptr; size_t d_data_cap = 0;
};

struct fskhip_xmodem_tx {
  fskhip_processor *p = nullptr;
  int device = 0;   // the processor's, kept here: destroy does not read the processor, which may be gone by then
  bool used = false;   // a send, poll, reset or state_set call has been made: no longer what create left (a remap or restore wants a fresh destination)
  XmTxState X{};
  XmTxScratch W{};
  uint32_t *d_totals = nullptr;
  // the packed file store: files are appended at `used`; a replaced file's bytes stay behind until the store is compacted
  uint8_t *d_store = nullptr; size_t store_cap = 0, store_used = 0;
  std::vector<uint32_t> h_off, h_len;   // each stream's file (h_len 0 and h_has 0: none)
  std::vector<uint8_t> h_has;
  uint32_t *d_new_off = nullptr; uint8_t *d_keep = nullptr;   // the compaction's arguments
  // staging for the _host form
  uint8_t *d_mask = nullptr, *d_abort = nullptr;
  uint32_t *d_streams = nullptr; size_t d_streams_cap = 0;
  fskhip_xmodem_tx_event *d_events = nullptr; size_t d_events_cap = 0;
};

struct fskhip_xmodem_recv {
  fskhip_processor *p = nullptr;
  int device = 0;   // the processor's, kept here: destroy does not read the processor, which may be gone by then
  bool used = false;   // a start, poll, reset, state_set or files_set call has been made: no longer what create left (a remap or restore wants a fresh destination)
  XmRecvState X{};
  XmRecvScratch W{};
  uint32_t *d_totals = nullptr;
  // staging for the _host forms
  uint8_t *d_mask = nullptr, *d_timeout = nullptr, *d_abort = nullptr;
  uint32_t *d_streams = nullptr;               // [n_streams] each, from create: no poll allocates
  fskhip_xmodem_recv_event *d_events = nullptr;
  uint32_t *d_sel = nullptr; size_t d_sel_cap = 0;
  uint64_t *d_offsets = nullptr; size_t d_offsets_cap = 0;
  uint8_t *d_packed = nullptr; size_t d_packed_cap = 0;
};
