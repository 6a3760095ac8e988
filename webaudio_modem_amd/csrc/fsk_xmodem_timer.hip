// fsk_xmodem_timer.hip -- the device half of fskhip_xmodem_recv_poll_timed_* / fskhip_xmodem_tx_poll_timed_* (include/fskhip_next.h):
// the wait timers of the resident file receiver and the resident sender, kept per stream in the engine's sample clock, around the
// polls as they are.  The rule is fsk_xmodem_timer.h's; nothing of it is restated here.
//
// Two launches around a poll, one lane per stream, 256 streams per workgroup, plain loads and stores, no atomics, no LDS:
//   fire  before the poll.  Reads what the poll's step kernel will read to select a stream (state, mask, tx_pending), moves the
//         stream's two words, and writes the flag byte the poll then takes -- the receiver's timeout[s], or the sender's abort[s]
//         with the caller's own abort[s] OR-ed in.  Every stream's two words as they were, what fire found the stream to be and
//         the ring's live byte count go to scratch.
//   arm   after the poll.  Reads the poll's third total first: a poll that stood down has every stream's two words put back, so
//         that a stood-down timed poll changes nothing.  Otherwise the streams fire found pending or waiting read their event
//         from the poll's scratch (the step kernel writes it for every selected stream, listed or not) and the ring's live count.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "fsk_launch.h"
#include "fsk_xmodem_timer.h"

namespace fsk {

namespace {

using namespace xw;

constexpr uint32_t kKindShift = 8u;   // saved[s]: the mark before fire in bits 0-7, what fire found (NOT_SELECTED ..) above

__global__ __launch_bounds__(256) void xm_timer_fire_kernel(XmTimerState W, const uint32_t *__restrict__ state, const uint32_t *__restrict__ tx_pending,
                                                            const uint32_t *__restrict__ rx_len, const uint8_t *__restrict__ mask,
                                                            const uint8_t *__restrict__ abort, uint32_t n_streams, uint32_t is_recv, uint32_t elapsed) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_streams) return;
  const uint32_t st = state[s];
  const bool sel = st != 0u && (!mask || mask[s] != 0);   // (IDLE is 0 in both handles)
  Words T{W.waited[s], W.mark[s]};
  W.old_waited[s] = T.waited;
  uint32_t kind = NOT_SELECTED, flag = 0u;
  if (sel) {
    const bool pending = tx_pending[s] != 0u;
    kind = pending ? PENDING : WAITING;
    W.saved[s] = T.mark | (kind << kKindShift);
    if (!pending) W.held[s] = rx_len[s];
    flag = fire(T, pending, is_recv && (st == FSKHIP_XR_SEND_NAK || st == FSKHIP_XR_SEND_ACK), elapsed, W.timeout_samples);
    W.waited[s] = T.waited;
    W.mark[s] = T.mark;
  } else {
    W.saved[s] = T.mark;
  }
  if (!is_recv && abort && abort[s] != 0) flag = 1u;   // a caller's abort still applies
  W.flag[s] = (uint8_t)flag;
}

// EV: fskhip_xmodem_recv_event or fskhip_xmodem_tx_event; both begin with status, state_after, control
template <class EV>
__global__ __launch_bounds__(256) void xm_timer_arm_kernel(XmTimerState W, const EV *__restrict__ ev, const uint32_t *__restrict__ rx_len,
                                                           const uint32_t *__restrict__ totals, uint32_t n_streams) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_streams) return;
  const uint32_t saved = W.saved[s];
  if (totals[2] == 0u) {   // the poll stood down (the same word for every lane of the grid): as if fire had not run
    W.waited[s] = W.old_waited[s];
    W.mark[s] = saved & 0xFFu;
    return;
  }
  const uint32_t kind = saved >> kKindShift;
  if (kind == NOT_SELECTED) return;
  Words T{W.waited[s], W.mark[s]};
  const Words was = T;
  const EV E = ev[s];
  if constexpr (std::is_same<EV, fskhip_xmodem_recv_event>::value)
    arm_recv(T, kind == WAITING, E.status, E.state_after, E.control, kind == WAITING ? W.held[s] : 0u, kind == WAITING ? rx_len[s] : 0u);
  else
    arm_tx(T, kind == WAITING, E.status, E.state_after, E.control, E.sent_len);
  if (T.waited != was.waited) W.waited[s] = T.waited;
  if (T.mark != was.mark) W.mark[s] = T.mark;
}

// The timers through remap, snapshot and restore (fskhip_xmodem_timer_remap / _snapshot / _restore): destination stream i takes
// the two words of source map[i] -- of i where map is null --, 0 and 0 where the entry is negative.  Either side is the pair of
// arrays (waited, mark) or, where TABLE, an interleaved record table (waited, mark per record; `waited` is its base, 8-byte
// aligned, `mark` unused).  The host has checked every entry against the source's count.
template <bool SRC_TABLE, bool DST_TABLE>
__global__ __launch_bounds__(256) void xm_timer_gather_kernel(uint32_t *__restrict__ dst_waited, uint32_t *__restrict__ dst_mark,
                                                              const uint32_t *__restrict__ src_waited, const uint32_t *__restrict__ src_mark,
                                                              const int64_t *__restrict__ map, uint32_t n_dst) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_dst) return;
  const int64_t m = map ? map[i] : (int64_t)i;
  uint2 T = make_uint2(0u, 0u);
  if (m >= 0) {
    if constexpr (SRC_TABLE) T = reinterpret_cast<const uint2 *>(src_waited)[m];
    else T = make_uint2(src_waited[m], src_mark[m]);
  }
  if constexpr (DST_TABLE) {
    reinterpret_cast<uint2 *>(dst_waited)[i] = T;
  } else {
    dst_waited[i] = T.x;
    dst_mark[i] = T.y;
  }
}

uint32_t groups_of(uint32_t n_streams) { return (n_streams + 255u) / 256u; }

}  // namespace

hipError_t launch_xmodem_timer_gather(const XmTimerState &D, const XmTimerState &S, const int64_t *d_map, uint32_t n_dst, hipStream_t st) {
  if (!n_dst) return hipSuccess;
  hipLaunchKernelGGL((xm_timer_gather_kernel<false, false>), dim3(groups_of(n_dst)), dim3(256), 0, st, D.waited, D.mark, S.waited, S.mark, d_map, n_dst);
  return hipGetLastError();
}

hipError_t launch_xmodem_timer_pack(const XmTimerState &S, const int64_t *d_sel, uint32_t n_sel, uint32_t *d_table, hipStream_t st) {
  if (!n_sel) return hipSuccess;
  hipLaunchKernelGGL((xm_timer_gather_kernel<false, true>), dim3(groups_of(n_sel)), dim3(256), 0, st, d_table, nullptr, S.waited, S.mark, d_sel, n_sel);
  return hipGetLastError();
}

hipError_t launch_xmodem_timer_unpack(const XmTimerState &D, const uint32_t *d_table, const int64_t *d_map, uint32_t n_dst, hipStream_t st) {
  if (!n_dst) return hipSuccess;
  hipLaunchKernelGGL((xm_timer_gather_kernel<true, false>), dim3(groups_of(n_dst)), dim3(256), 0, st, D.waited, D.mark, d_table, nullptr, d_map, n_dst);
  return hipGetLastError();
}

hipError_t launch_xmodem_timer_fire(const XmTimerState &W, bool is_recv, const uint32_t *d_state, const ProcState &T, uint32_t n_streams, const uint8_t *d_mask,
                                    const uint8_t *d_abort, uint32_t elapsed, hipStream_t st) {
  if (!n_streams) return hipSuccess;
  hipLaunchKernelGGL(xm_timer_fire_kernel, dim3(groups_of(n_streams)), dim3(256), 0, st, W, d_state, T.tx_pending, T.rx_len, d_mask, d_abort, n_streams,
                     is_recv ? 1u : 0u, elapsed);
  return hipGetLastError();
}

hipError_t launch_xmodem_timer_arm_recv(const XmTimerState &W, const fskhip_xmodem_recv_event *d_ev, const ProcState &T, uint32_t n_streams,
                                        const uint32_t *d_totals, hipStream_t st) {
  if (!n_streams) return hipSuccess;
  hipLaunchKernelGGL(xm_timer_arm_kernel<fskhip_xmodem_recv_event>, dim3(groups_of(n_streams)), dim3(256), 0, st, W, d_ev, T.rx_len, d_totals, n_streams);
  return hipGetLastError();
}

hipError_t launch_xmodem_timer_arm_tx(const XmTimerState &W, const fskhip_xmodem_tx_event *d_ev, const ProcState &T, uint32_t n_streams,
                                      const uint32_t *d_totals, hipStream_t st) {
  if (!n_streams) return hipSuccess;
  hipLaunchKernelGGL(xm_timer_arm_kernel<fskhip_xmodem_tx_event>, dim3(groups_of(n_streams)), dim3(256), 0, st, W, d_ev, T.rx_len, d_totals, n_streams);
  return hipGetLastError();
}

}  // namespace fsk
