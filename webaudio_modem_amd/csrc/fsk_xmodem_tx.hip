// fsk_xmodem_tx.hip -- the device half of fskhip_xmodem_tx_poll_host / _device (include/fskhip_next.h): XModemTransport's send
// side, one demodulate() reply per poll.  A poll takes the whole content of every waiting stream's RX ring as that reply, applies
// the state's wait to it (fsk_xmodem_tx_step.h), builds the packet or the EOT the reference would modulate next into a staging
// slab and lists the streams where something happened, in the compacted drain's form (fsk_drain.hip).  The caller follows the
// commit with launch_processor_tx_start over the slab on the same stream; nothing crosses to the host.
//
// Three launches, no atomics:
//   step    one lane per stream, 256 streams per workgroup.  A selected stream (mask, state not IDLE) that is neither aborted nor
//           still modulating has its live ring bytes searched for the first of ACK / NAK / EOT, or for any ACK.  Rings whose
//           capacity is a multiple of 16 are staged through LDS in 64-byte tiles per lane exactly as xm_rx_scan_kernel stages them
//           (fsk_xmodem_rx.hip): four 16-byte loads per lane, 16 rows x 64 B each, from the chunk that holds readIndex, wrapping at
//           the ring's end; a lane stops looking once its wait is settled, a wave stops loading once all its lanes are.  Other
//           capacities are read byte by byte.  The event, three flag bits, the kind of transmission and the retransmission count
//           go to scratch, the transmit mask of every stream is cleared, and nothing else is written.  The workgroup reduces its
//           listed streams to one pair (fsk_pick_dev.h); the byte half of the pair is always 0.
//   totals  the drain's scan kernel as it is (launch_drain_totals): pairs -> exclusive positions + {n_events, 0, fits}.
//   commit  reads the totals first and stands down as a whole when the cap is too small: the transmit mask stays clear, so the
//           launch_processor_tx_start behind it starts nothing.  Otherwise it writes streams[] and events[], builds the packets --
//           the header as one dword, the fragment moved as a span with consecutive lanes on consecutive bytes as drain_pack_kernel
//           moves its rings, the CRC by the owning lane with the table step of fsk_xmodem_scan.h --, sets the slab's lengths and
//           mask, empties the rings that gave their reply and updates the sender words.
// A wave none of whose lanes transmits a packet builds no CRC table and moves nothing.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_launch.h"
#include "fsk_params.h"
#include "fsk_pick_dev.h"
#include "fsk_xmodem_tx_step.h"

namespace fsk {

namespace {

using namespace xt;

constexpr uint32_t kInFlight = 4;   // span passes whose loads are issued before the first store
// flag word of a stream: bit 0 a sender word changes, bit 1 listed, bit 2 the ring is emptied; bits 4-5 SEND_*; bits 8-9 the
// retransmission count's increase (0..2)
constexpr uint32_t kTouched = 1u, kListed = 2u, kDrained = 4u, kSendShift = 4u, kRetxShift = 8u;

// orders this wave's LDS traffic against itself: what its lanes wrote before is what they read after
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o, 64));
  return x;
}

// byte `pos` (<= cap) of the span that starts at index r (< cap) of a ring of cap bytes
__device__ __forceinline__ uint32_t ring_index(uint32_t r, uint32_t cap, uint32_t pos) {
  const uint32_t room = cap - r;
  return pos < room ? r + pos : pos - room;
}

template <bool VEC16>
__global__ __launch_bounds__(256) void xm_tx_step_kernel(ProcState T, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ abort, uint32_t n_streams,
                                                         XmTxState X, fskhip_xmodem_tx_event *__restrict__ ev, uint32_t *__restrict__ flags,
                                                         uint8_t *__restrict__ tx_mask, uint2 *__restrict__ pairs) {
  __shared__ uint32_t ws[4][2];
  __shared__ uint4 stages[4][VEC16 ? 4 * 65 : 1];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cap = T.rx_cap;
  const bool valid = s < n_streams;
  const uint32_t st = valid ? X.state[s] : (uint32_t)FSKHIP_XT_IDLE;
  const bool sel = valid && st != FSKHIP_XT_IDLE && (!mask || mask[s] != 0);
  const bool ab = sel && abort && abort[s] != 0;
  const bool pending = sel && !ab && T.tx_pending[s] != 0u;
  const bool look = sel && !ab && !pending;
  const uint32_t n = look ? T.rx_len[s] : 0u;
  Find F;
  F.init();
  if (__builtin_amdgcn_ballot_w64(n > 0u) != 0ull) {   // (the same for every lane of the wave)
    const uint32_t r = n ? T.rx_r[s] : 0u;
    if (VEC16) {
      // the row as 16-byte chunks from the one that holds readIndex: the span is bytes [skew, skew + n) of that chunk sequence
      uint4 *stage = stages[wv];
      const uint32_t n_chunks = cap >> 4, r16 = r >> 4, skew = r & 15u;
      const uint32_t need = n ? skew + n : 0u;
      const uint32_t sub_row = lane >> 2, chunk = lane & 3u;
      const size_t row0 = (size_t)blockIdx.x * 256u + 64u * wv;
      for (uint32_t t0 = 0;; t0 += 64u) {
        const uint32_t want = (t0 < need && !F.settled(st)) ? need : 0u;   // 0: this lane's row needs no further tile
        if (wave_max(want) == 0u) break;
        wave_sync();   // (the tile before this one has been read)
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
          const uint32_t row = 16u * i + sub_row;
          const uint32_t row_r16 = (uint32_t)__shfl((int)r16, (int)row, 64), row_need = (uint32_t)__shfl((int)want, (int)row, 64);
          const uint32_t j = (t0 >> 4) + chunk;
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (j * 16u < row_need) {   // j <= n_chunks here, so one subtraction wraps it; row_need is 0 for a row past the batch
            uint32_t c = row_r16 + j;
            if (c >= n_chunks) c -= n_chunks;
            v = *reinterpret_cast<const uint4 *>(T.rx_buf + (row0 + row) * cap + (size_t)c * 16u);
          }
          stage[chunk * 65u + row] = v;
        }
        wave_sync();
        if (want) {
#pragma unroll 1
          for (uint32_t c = 0; c < 4u; c++) {
            const uint32_t at = t0 + 16u * c;
            if (at >= need || F.settled(st)) break;
            const uint4 v = stage[c * 65u + lane];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint32_t lo = at < skew ? skew - at : 0u, hi = need - at < 16u ? need - at : 16u;
            F.quad(w, lo < 16u ? lo : 16u, hi);
          }
        }
      }
    } else if (n) {
      const uint8_t *row = T.rx_buf + (size_t)s * cap;
      for (uint32_t pos = 0; pos < n && !F.settled(st); pos++) F.byte(row[ring_index(r, cap, pos)]);
    }
  }
  uint32_t f = 0u;
  if (sel) {
    Words W{st, X.sequence[s], X.index[s], X.n_fragments[s], X.retries[s], 0u, 0u};
    const Step R = step(W, ab, pending, F, X.max_retries, X.file_len[s], X.max_payload);
    ev[s] = R.ev;
    f = (R.touched ? kTouched : 0u) | (R.listed ? kListed : 0u) | (R.drained ? kDrained : 0u) | (R.send << kSendShift) | (W.retransmitted << kRetxShift);
  }
  if (valid) { flags[s] = f; tx_mask[s] = 0u; }
  const Pick P = pick_scan((f & kListed) != 0u, 0u, ws);
  if (threadIdx.x == 0u) pairs[blockIdx.x] = make_uint2(P.tot_s, 0u);
}

__global__ __launch_bounds__(256) void xm_tx_commit_kernel(ProcState T, uint32_t n_streams, XmTxState X, const fskhip_xmodem_tx_event *__restrict__ ev,
                                                           const uint32_t *__restrict__ flags, const uint2 *__restrict__ pairs,
                                                           const uint32_t *__restrict__ totals, uint8_t *__restrict__ slab, uint32_t slab_pitch,
                                                           uint32_t *__restrict__ tx_lens, uint8_t *__restrict__ tx_mask, uint32_t *__restrict__ streams,
                                                           fskhip_xmodem_tx_event *__restrict__ events) {
  __shared__ uint32_t ws[4][2];
  __shared__ uint32_t tables[4][256];
  __shared__ SpanJob jobs[4][64];
  if (totals[2] == 0u) return;   // the cap is too small: nothing is committed (the same word for every lane of the grid)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t f = s < n_streams ? flags[s] : 0u;
  const bool touched = (f & kTouched) != 0u, listed = (f & kListed) != 0u;
  const uint32_t send = (f >> kSendShift) & 3u;
  fskhip_xmodem_tx_event E{};
  if (touched) E = ev[s];
  const Pick P = pick_scan(listed, 0u, ws);
  const uint2 base = pairs[blockIdx.x];
  if (listed) {
    streams[base.x + P.pos_s] = s;
    events[base.x + P.pos_s] = E;
  }
  uint8_t *row = slab + (size_t)(send ? s : 0u) * slab_pitch;
  const bool packet = send == SEND_PACKET;
  if (__builtin_amdgcn_ballot_w64(packet) != 0ull) {   // (the same for every lane of the wave)
    uint32_t *table = tables[wv];
    for (uint32_t i = lane; i < 256u; i += 64u) table[i] = xm::crc_table_entry(i);
    const uint32_t len = packet ? E.sent_len - 6u : 0u;   // (sent_len of a packet is its fragment's length + 6)
    const uint32_t src = packet ? X.file_off[s] + E.fragment_index * X.max_payload : 0u;
    const uint64_t vote = __builtin_amdgcn_ballot_w64(packet && len > 0u);
    const uint32_t n_jobs = (uint32_t)__builtin_popcountll(vote);
    if (packet && len > 0u) jobs[wv][__builtin_popcountll(vote & ((1ull << lane) - 1ull))] = SpanJob{s, src, len, 0u};
    const uint32_t longest = wave_max(len);
    wave_sync();
    // the fragments: consecutive lanes on consecutive bytes of one span, to byte 4 of the stream's slab row
    const uint32_t lps = lanes_per_span(longest), spp = 64u / lps;   // lanes per span, spans per pass
    const uint32_t sub = lane / lps, k0 = lane % lps;
    for (uint32_t p = 0; p < n_jobs; p += spp * kInFlight) {
      SpanJob J[kInFlight];
      uint32_t most = 0u;
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++) {
        const uint32_t slot = p + u * spp + sub;
        J[u] = slot < n_jobs ? jobs[wv][slot] : SpanJob{0u, 0u, 0u, 0u};
        most = max(most, J[u].len);
      }
      for (uint32_t k = k0; k < most; k += lps) {
        uint8_t v[kInFlight];
#pragma unroll
        for (uint32_t u = 0; u < kInFlight; u++)
          if (k < J[u].len) v[u] = X.store[(size_t)J[u].start + k];
#pragma unroll
        for (uint32_t u = 0; u < kInFlight; u++)
          if (k < J[u].len) slab[(size_t)J[u].src * slab_pitch + 4u + k] = v[u];
      }
    }
    if (packet) {   // SOH seq ~seq len | payload | crc_hi crc_lo, the CRC over the payload only (packet.ts:21-53)
      uint32_t crc = 0xFFFFu;
      for (uint32_t k = 0; k < len; k++) crc = xm::crc_step(table, crc, X.store[(size_t)src + k]);
      *reinterpret_cast<uint32_t *>(row) = xm::kSOH | (E.sequence << 8) | ((255u - E.sequence) << 16) | (len << 24);   // (rows are 16-byte aligned)
      row[4u + len] = (uint8_t)(crc >> 8);
      row[5u + len] = (uint8_t)(crc & 0xFFu);
    }
  }
  if (send == SEND_EOT) row[0] = (uint8_t)kEOT;
  if (send) { tx_lens[s] = E.sent_len; tx_mask[s] = 1u; }
  if (f & kDrained) {   // the reply is everything buffered: readIndex advanced by _length modulo the capacity, _length = 0
    const uint32_t held = T.rx_len[s];
    if (held) { T.rx_r[s] = ring_index(T.rx_r[s], T.rx_cap, held); T.rx_len[s] = 0u; }
  }
  if (touched) {
    X.state[s] = E.state_after; X.sequence[s] = E.sequence; X.index[s] = E.fragment_index; X.retries[s] = E.retries;
    if (send) X.sent[s] += 1u;
    const uint32_t retx = (f >> kRetxShift) & 3u;
    if (retx) X.retransmitted[s] += retx;
  }
}

// files of some streams into a new packed store: one wave per stream, consecutive lanes on consecutive bytes
__global__ __launch_bounds__(256) void xm_tx_repack_kernel(const uint8_t *__restrict__ old_store, const uint32_t *__restrict__ old_off,
                                                           const uint32_t *__restrict__ new_off, const uint32_t *__restrict__ lens,
                                                           const uint8_t *__restrict__ keep, uint32_t n_streams, uint8_t *__restrict__ new_store) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (s >= n_streams || !keep[s]) return;
  const uint32_t n = lens[s];
  const uint8_t *src = old_store + old_off[s];
  uint8_t *dst = new_store + new_off[s];
  for (uint32_t k = lane; k < n; k += 64u) dst[k] = src[k];
}

uint32_t groups_of(uint32_t n_streams) { return n_streams ? (n_streams + 255u) / 256u : 1u; }   // (an empty batch still writes its totals)

}  // namespace

size_t xmodem_tx_pair_words(uint32_t n_streams) { return 2u * (size_t)groups_of(n_streams); }

hipError_t launch_xmodem_tx_step(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, const uint8_t *d_abort, const XmTxState &X, const XmTxScratch &W,
                                 uint32_t cap_streams, uint32_t *d_totals, hipStream_t st) {
  const uint32_t groups = groups_of(n_streams);
  if ((T.rx_cap & 15u) == 0u)
    hipLaunchKernelGGL(xm_tx_step_kernel<true>, dim3(groups), dim3(256), 0, st, T, d_mask, d_abort, n_streams, X, W.ev, W.flags, W.tx_mask, (uint2 *)W.pairs);
  else
    hipLaunchKernelGGL(xm_tx_step_kernel<false>, dim3(groups), dim3(256), 0, st, T, d_mask, d_abort, n_streams, X, W.ev, W.flags, W.tx_mask, (uint2 *)W.pairs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_drain_totals(W.pairs, groups, cap_streams, 0u, d_totals, st);
}

hipError_t launch_xmodem_tx_commit(const ProcState &T, uint32_t n_streams, const XmTxState &X, const XmTxScratch &W, const uint32_t *d_totals, uint32_t *d_streams,
                                   fskhip_xmodem_tx_event *d_events, hipStream_t st) {
  hipLaunchKernelGGL(xm_tx_commit_kernel, dim3(groups_of(n_streams)), dim3(256), 0, st, T, n_streams, X, W.ev, W.flags, (const uint2 *)W.pairs, d_totals, W.slab,
                     W.slab_pitch, W.tx_lens, W.tx_mask, d_streams, d_events);
  return hipGetLastError();
}

hipError_t launch_xmodem_tx_repack(const uint8_t *d_old_store, const uint32_t *d_old_off, const uint32_t *d_new_off, const uint32_t *d_lens, const uint8_t *d_keep,
                                   uint32_t n_streams, uint8_t *d_new_store, hipStream_t st) {
  if (!n_streams) return hipSuccess;
  hipLaunchKernelGGL(xm_tx_repack_kernel, dim3((n_streams + 3u) / 4u), dim3(256), 0, st, d_old_store, d_old_off, d_new_off, d_lens, d_keep, n_streams, d_new_store);
  return hipGetLastError();
}

}  // namespace fsk
