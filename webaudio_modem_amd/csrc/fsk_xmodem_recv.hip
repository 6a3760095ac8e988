// fsk_xmodem_recv.hip -- the device half of fskhip_xmodem_recv_poll_host / _device (include/fskhip_next.h): XModemTransport's
// receiveData(), one reply-owing step per poll.  A poll walks every waiting stream's RX ring in place with the shared receive
// grammar (fsk_xmodem_scan.h) up to the first step the receiver answers, applies the transition (fsk_xmodem_recv_step.h), appends
// an accepted payload to the stream's file row, builds the ACK / NAK byte into a staging slab and lists the streams where
// something happened, in the compacted drain's form (fsk_drain.hip).  The caller follows the commit with
// launch_processor_tx_start over the slab on the same stream; no ring byte, file byte or control byte crosses to the host.
//
// Three launches, no atomics:
//   step    one lane per stream, 256 streams per workgroup.  A selected stream (mask, state not IDLE) that is neither aborted nor
//           still modulating is walked from readIndex.  Rings whose capacity is a multiple of 16 are staged through LDS in 64-byte
//           tiles per lane exactly as xm_rx_scan_kernel and xm_tx_step_kernel stage them: four 16-byte loads per lane, 16 rows x
//           64 B each, from the chunk that holds readIndex, wrapping at the ring's end; a lane stops reading once its reply-owing
//           step is found, a wave stops loading once all its lanes have stopped.  Other capacities are read byte by byte.  Each
//           wave keeps its own CRC table; a wave with no lane to walk builds none.  The event, the flag bits, the bytes to remove
//           and the payload span go to scratch, the transmit mask of every stream is cleared, and nothing else is written.  The
//           workgroup reduces its listed streams to one pair (fsk_pick_dev.h); the byte half of the pair is always 0.
//   totals  the drain's scan kernel as it is (launch_drain_totals): pairs -> exclusive positions + {n_events, 0, fits}.
//   commit  reads the totals first and stands down as a whole when the cap is too small: the transmit mask stays clear, so the
//           launch_processor_tx_start behind it starts nothing.  Otherwise it writes streams[] and events[], moves the accepted
//           payload spans from ring to file row as drain_pack_kernel moves its rings -- consecutive lanes on consecutive bytes of
//           one span, ring wrap handled, four passes' loads before the first store --, advances the rings, updates the words and
//           writes the control byte, length 1 and mask into the slab.
// files: the assembled files of some streams to or from one packed buffer, one wave per stream, consecutive lanes on consecutive bytes.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_launch.h"
#include "fsk_params.h"
#include "fsk_pick_dev.h"
#include "fsk_xmodem_recv_step.h"

namespace fsk {

namespace {

using namespace xm;

constexpr uint32_t kInFlight = 4;   // span passes whose loads are issued before the first store
// flag word of a stream: a receiver or ring word changes; listed; packets_received / dropped go up by one; a control byte is
// transmitted; an accepted payload is appended
constexpr uint32_t kTouched = 1u, kListed = 2u, kPacket = 4u, kDropped = 8u, kSend = 16u, kAppend = 32u;

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
__global__ __launch_bounds__(256) void xm_recv_step_kernel(ProcState T, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ timeout,
                                                           const uint8_t *__restrict__ abort, uint32_t n_streams, XmRecvState X,
                                                           fskhip_xmodem_recv_event *__restrict__ ev, uint32_t *__restrict__ flags,
                                                           uint32_t *__restrict__ removed, uint32_t *__restrict__ span, uint8_t *__restrict__ tx_mask,
                                                           uint2 *__restrict__ pairs) {
  __shared__ uint32_t ws[4][2];
  __shared__ uint32_t tables[4][256];
  __shared__ uint4 stages[4][VEC16 ? 4 * 65 : 1];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cap = T.rx_cap;
  const bool valid = s < n_streams;
  const uint32_t st = valid ? X.state[s] : (uint32_t)FSKHIP_XR_IDLE;
  const bool sel = valid && st != FSKHIP_XR_IDLE && (!mask || mask[s] != 0);
  const bool ab = sel && abort && abort[s] != 0;
  const bool pending = sel && !ab && T.tx_pending[s] != 0u;
  const bool look = sel && !ab && !pending;
  const uint32_t n = look ? T.rx_len[s] : 0u;
  Scan sc;
  sc.init(look ? X.expected[s] : 1u);
  if (__builtin_amdgcn_ballot_w64(n > 0u) != 0ull) {   // (the same for every lane of the wave)
    uint32_t *table = tables[wv];
    for (uint32_t i = lane; i < 256u; i += 64u) table[i] = crc_table_entry(i);
    wave_sync();
    const uint32_t r = n ? T.rx_r[s] : 0u;
    if (VEC16) {
      // the row as 16-byte chunks from the one that holds readIndex: the span is bytes [skew, skew + n) of that chunk sequence
      uint4 *stage = stages[wv];
      const uint32_t n_chunks = cap >> 4, r16 = r >> 4, skew = r & 15u;
      const uint32_t need = n ? skew + n : 0u;
      const uint32_t sub_row = lane >> 2, chunk = lane & 3u;
      const size_t row0 = (size_t)blockIdx.x * 256u + 64u * wv;
      for (uint32_t t0 = 0;; t0 += 64u) {
        const uint32_t want = (t0 < need && !sc.owes_reply()) ? need : 0u;   // 0: this lane's row needs no further tile
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
            const uint4 v = stage[c * 65u + lane];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 16; q++) {
              const uint32_t off = t0 + 16u * c + (uint32_t)q;
              if (off >= skew && off < need && !sc.owes_reply())
                sc.byte<false>(table, (w[q >> 2] >> ((q & 3) * 8)) & 0xFFu, off - skew, nullptr, 0);
            }
          }
        }
      }
    } else if (n) {
      const uint8_t *row = T.rx_buf + (size_t)s * cap;
      for (uint32_t pos = 0; pos < n && !sc.owes_reply(); pos++) sc.byte<false>(table, row[ring_index(r, cap, pos)], pos, nullptr, 0);
    }
  }
  uint32_t f = 0u;
  if (sel) {
    xr::Words W{st, X.expected[s], X.retries[s], X.file_len[s], 0u, 0u, 0u};
    const xr::Step R = xr::step(W, ab, pending, look && timeout && timeout[s] != 0, xr::found_of(sc), n, X.max_retries, X.file_cap);
    ev[s] = R.ev;
    removed[s] = R.removed;
    span[s] = R.span;
    f = (R.touched ? kTouched : 0u) | (R.listed ? kListed : 0u) | (W.packets ? kPacket : 0u) | (W.dropped ? kDropped : 0u) | (W.sent ? kSend : 0u) |
        (R.appended ? kAppend : 0u);
  }
  if (valid) { flags[s] = f; tx_mask[s] = 0u; }
  const Pick P = pick_scan((f & kListed) != 0u, 0u, ws);
  if (threadIdx.x == 0u) pairs[blockIdx.x] = make_uint2(P.tot_s, 0u);
}

__global__ __launch_bounds__(256) void xm_recv_commit_kernel(ProcState T, uint32_t n_streams, XmRecvState X, const fskhip_xmodem_recv_event *__restrict__ ev,
                                                             const uint32_t *__restrict__ flags, const uint32_t *__restrict__ removed,
                                                             const uint32_t *__restrict__ span, const uint2 *__restrict__ pairs,
                                                             const uint32_t *__restrict__ totals, uint8_t *__restrict__ slab, uint32_t slab_pitch,
                                                             uint32_t *__restrict__ tx_lens, uint8_t *__restrict__ tx_mask, uint32_t *__restrict__ streams,
                                                             fskhip_xmodem_recv_event *__restrict__ events) {
  __shared__ uint32_t ws[4][2];
  __shared__ SpanJob jobs[4][64];
  if (totals[2] == 0u) return;   // the cap is too small: nothing is committed (the same word for every lane of the grid)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cap = T.rx_cap;
  const uint32_t f = s < n_streams ? flags[s] : 0u;
  const bool touched = (f & kTouched) != 0u, listed = (f & kListed) != 0u;
  fskhip_xmodem_recv_event E{};
  if (touched) E = ev[s];
  const Pick P = pick_scan(listed, 0u, ws);
  const uint2 base = pairs[blockIdx.x];
  if (listed) {
    streams[base.x + P.pos_s] = s;
    events[base.x + P.pos_s] = E;
  }
  const uint32_t r = touched ? T.rx_r[s] : 0u;
  const uint32_t held = touched ? T.rx_len[s] : 0u;
  // the accepted payloads: ring -> file row, at the file's length before this poll
  const uint32_t len = (f & kAppend) ? E.accepted_len : 0u;
  const uint64_t vote = __builtin_amdgcn_ballot_w64(len > 0u);
  if (vote != 0ull) {   // (the same for every lane of the wave)
    const uint32_t n_jobs = (uint32_t)__builtin_popcountll(vote);
    if (len > 0u) jobs[wv][__builtin_popcountll(vote & ((1ull << lane) - 1ull))] = SpanJob{s, ring_index(r, cap, span[s]), len, E.file_len - len};
    const uint32_t longest = wave_max(len);
    wave_sync();
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
          if (k < J[u].len) v[u] = T.rx_buf[(size_t)J[u].src * cap + ring_index(J[u].start, cap, k)];
#pragma unroll
        for (uint32_t u = 0; u < kInFlight; u++)
          if (k < J[u].len) X.files[(size_t)J[u].src * X.file_cap + J[u].dst + k] = v[u];
      }
    }
  }
  if (touched) {   // readIndex advanced by what left the ring, modulo the capacity; writeIndex and the bytes stay
    const uint32_t gone = removed[s] <= held ? removed[s] : held;
    if (gone) { T.rx_r[s] = ring_index(r, cap, gone); T.rx_len[s] = held - gone; }
    X.state[s] = E.state_after; X.expected[s] = E.expected; X.retries[s] = E.retries; X.file_len[s] = E.file_len;
    if (f & kPacket) X.packets[s] += 1u;
    if (f & kDropped) X.dropped[s] += 1u;
    if (f & kSend) {   // the 'modulate' request: one byte
      X.sent[s] += 1u;
      slab[(size_t)s * slab_pitch] = (uint8_t)E.control;
      tx_lens[s] = 1u;
      tx_mask[s] = 1u;
    }
  }
}

// PACK: the file rows of streams sel[0 .. n_sel) -> packed[offsets[i] .. offsets[i+1]); otherwise the other way, and file_len set
template <bool PACK>
__global__ __launch_bounds__(256) void xm_recv_files_kernel(uint8_t *__restrict__ files, uint32_t file_cap, uint32_t *__restrict__ file_len,
                                                            const uint32_t *__restrict__ sel, const uint64_t *__restrict__ offsets, uint32_t n_sel,
                                                            uint8_t *__restrict__ packed) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= n_sel) return;
  const uint64_t off = offsets[i];
  const uint32_t n = (uint32_t)(offsets[i + 1] - off);
  uint8_t *row = files + (size_t)sel[i] * file_cap;
  uint8_t *flat = packed + off;
  if (PACK) {
    for (uint32_t k = lane; k < n; k += 64u) flat[k] = row[k];
  } else {
    for (uint32_t k = lane; k < n; k += 64u) row[k] = flat[k];
    if (lane == 0u) file_len[sel[i]] = n;
  }
}

uint32_t groups_of(uint32_t n_streams) { return n_streams ? (n_streams + 255u) / 256u : 1u; }   // (an empty batch still writes its totals)

}  // namespace

size_t xmodem_recv_pair_words(uint32_t n_streams) { return 2u * (size_t)groups_of(n_streams); }

hipError_t launch_xmodem_recv_step(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, const uint8_t *d_timeout, const uint8_t *d_abort,
                                   const XmRecvState &X, const XmRecvScratch &W, uint32_t cap_streams, uint32_t *d_totals, hipStream_t st) {
  const uint32_t groups = groups_of(n_streams);
  if ((T.rx_cap & 15u) == 0u)
    hipLaunchKernelGGL(xm_recv_step_kernel<true>, dim3(groups), dim3(256), 0, st, T, d_mask, d_timeout, d_abort, n_streams, X, W.ev, W.flags, W.removed, W.span,
                       W.tx_mask, (uint2 *)W.pairs);
  else
    hipLaunchKernelGGL(xm_recv_step_kernel<false>, dim3(groups), dim3(256), 0, st, T, d_mask, d_timeout, d_abort, n_streams, X, W.ev, W.flags, W.removed, W.span,
                       W.tx_mask, (uint2 *)W.pairs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_drain_totals(W.pairs, groups, cap_streams, 0u, d_totals, st);
}

hipError_t launch_xmodem_recv_commit(const ProcState &T, uint32_t n_streams, const XmRecvState &X, const XmRecvScratch &W, const uint32_t *d_totals,
                                     uint32_t *d_streams, fskhip_xmodem_recv_event *d_events, hipStream_t st) {
  hipLaunchKernelGGL(xm_recv_commit_kernel, dim3(groups_of(n_streams)), dim3(256), 0, st, T, n_streams, X, W.ev, W.flags, W.removed, W.span,
                     (const uint2 *)W.pairs, d_totals, W.slab, W.slab_pitch, W.tx_lens, W.tx_mask, d_streams, d_events);
  return hipGetLastError();
}

hipError_t launch_xmodem_recv_files(bool pack, const XmRecvState &X, const uint32_t *d_sel, const uint64_t *d_offsets, uint32_t n_sel, uint8_t *d_packed,
                                    hipStream_t st) {
  if (!n_sel) return hipSuccess;
  if (pack)
    hipLaunchKernelGGL(xm_recv_files_kernel<true>, dim3((n_sel + 3u) / 4u), dim3(256), 0, st, X.files, X.file_cap, X.file_len, d_sel, d_offsets, n_sel, d_packed);
  else
    hipLaunchKernelGGL(xm_recv_files_kernel<false>, dim3((n_sel + 3u) / 4u), dim3(256), 0, st, X.files, X.file_cap, X.file_len, d_sel, d_offsets, n_sel, d_packed);
  return hipGetLastError();
}

}  // namespace fsk
