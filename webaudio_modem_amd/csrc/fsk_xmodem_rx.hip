// fsk_xmodem_rx.hip -- the device half of fskhip_xmodem_rx_poll_host / _device (include/fskhip_next.h): XModemTransport's receive
// grammar run over the FSKProcessor RX rings where they are.  Each ring is walked in place from readIndex, only whole grammar steps
// leave it, and what crosses to the caller is the accepted payloads plus one result record per stream with something to answer, in
// the compacted drain's CSR form (fsk_drain.hip).
//
// Three launches, no atomics:
//   scan    one lane per stream, 256 streams per workgroup.  A selected stream (mask, ring not empty) is walked with the shared
//           state machine (fsk_xmodem_scan.h); its result R', the bytes to take out and two flag bits go to scratch and nothing
//           else is written.  Rings whose capacity is a multiple of 16 are staged through LDS in 64-byte tiles per lane -- four
//           16-byte loads per lane, 16 rows x 64 B each, chunk-major with a one-slot pad, as scan_tiled_kernel stages its rows
//           (fsk_xmodem.hip) -- with each row's tiles starting at the 16-byte chunk that holds readIndex and wrapping at the ring's
//           end; chunks past a row's live span are not loaded.  Other capacities are read byte by byte.  Every wave keeps its own
//           CRC table and tile stage and synchronises with itself only, so a wave none of whose lanes is selected skips all of
//           it: it reads its length words, writes its flags and joins the workgroup's count.  The workgroup reduces
//           {listed streams, payload bytes} to one pair exactly as the drain's count kernel does (fsk_pick_dev.h).
//   totals  the drain's scan kernel as it is (launch_drain_totals): pairs -> exclusive positions + {n_events, n_bytes, fits}.
//   commit  reads the totals first and stands down as a whole when a cap is too small.  Otherwise it writes streams[], results[],
//           offsets[], copies the accepted payloads, advances the rings and updates expected / packets / dropped.  For the payloads
//           the lane of a listed stream walks its packet HEADERS only (the scan pass has checked the CRCs), 6 + len at a time,
//           and posts one payload span per round to LDS; the wave then moves the posted spans as drain_pack_kernel moves its
//           rings: consecutive lanes on consecutive bytes of one span, ring wrap handled, four passes' loads before the first store.
// The limiter is expected to be the serial byte walk of the busiest lane of a wave (the CRC is a dependent chain), not memory.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_launch.h"
#include "fsk_params.h"
#include "fsk_pick_dev.h"
#include "fsk_xmodem_scan.h"

namespace fsk {

namespace {

using namespace xm;

constexpr uint32_t kInFlight = 4;       // span passes whose loads are issued before the first store
constexpr uint32_t kTouched = 1u, kListed = 2u;   // flag bits of a stream: selected (ring and state are updated); has an event

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

// byte `pos` (< cap) of the span that starts at index r (< cap) of a ring of cap bytes
__device__ __forceinline__ uint32_t ring_index(uint32_t r, uint32_t cap, uint32_t pos) {
  const uint32_t room = cap - r;
  return pos < room ? r + pos : pos - room;
}

template <bool VEC16>
__global__ __launch_bounds__(256) void xm_rx_scan_kernel(ProcState T, const uint8_t *__restrict__ mask, uint32_t n_streams,
                                                         const uint32_t *__restrict__ expected, fskhip_xmodem_result *__restrict__ res,
                                                         uint32_t *__restrict__ removed, uint32_t *__restrict__ flags, uint2 *__restrict__ pairs) {
  __shared__ uint32_t ws[4][2];
  __shared__ uint32_t tables[4][256];
  __shared__ uint4 stages[4][VEC16 ? 4 * 65 : 1];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cap = T.rx_cap;
  const bool valid = s < n_streams;
  const uint32_t held = valid ? T.rx_len[s] : 0u;
  const bool sel = valid && held > 0u && (!mask || mask[s] != 0);
  bool listed = false;
  uint32_t data_len = 0u;
  if (__builtin_amdgcn_ballot_w64(sel) != 0ull) {   // (the same for every lane of the wave)
    uint32_t *table = tables[wv];
    for (uint32_t i = lane; i < 256u; i += 64u) table[i] = crc_table_entry(i);
    wave_sync();
    const uint32_t n = sel ? held : 0u;
    const uint32_t r = sel ? T.rx_r[s] : 0u;
    Scan sc;
    sc.init(sel ? expected[s] : 1u);
    if (VEC16) {
      // the row as 16-byte chunks from the one that holds readIndex: the span is bytes [skew, skew + n) of that chunk sequence
      uint4 *stage = stages[wv];
      const uint32_t n_chunks = cap >> 4, r16 = r >> 4, skew = r & 15u;
      const uint32_t need = sel ? skew + n : 0u;
      const uint32_t need_max = wave_max(need);
      const uint32_t sub_row = lane >> 2, chunk = lane & 3u;
      const size_t row0 = (size_t)blockIdx.x * 256u + 64u * wv;
      for (uint32_t t0 = 0; t0 < need_max; t0 += 64u) {
        wave_sync();   // (the tile before this one has been read)
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
          const uint32_t row = 16u * i + sub_row;
          const uint32_t row_r16 = (uint32_t)__shfl((int)r16, (int)row, 64), row_need = (uint32_t)__shfl((int)need, (int)row, 64);
          const uint32_t j = (t0 >> 4) + chunk;
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (j * 16u < row_need) {   // j <= n_chunks here, so one subtraction wraps it
            uint32_t c = row_r16 + j;
            if (c >= n_chunks) c -= n_chunks;
            v = *reinterpret_cast<const uint4 *>(T.rx_buf + (row0 + row) * cap + (size_t)c * 16u);
          }
          stage[chunk * 65u + row] = v;
        }
        wave_sync();
        if (t0 < need && sc.state != ST_DONE) {
#pragma unroll 1
          for (uint32_t c = 0; c < 4u; c++) {
            const uint4 v = stage[c * 65u + lane];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 16; q++) {
              const uint32_t off = t0 + 16u * c + (uint32_t)q;
              if (off >= skew && off < need && sc.state != ST_DONE)
                sc.byte<false>(table, (w[q >> 2] >> ((q & 3) * 8)) & 0xFFu, off - skew, nullptr, 0);
            }
          }
        }
      }
    } else {
      const uint8_t *row = T.rx_buf + (size_t)s * cap;
      for (uint32_t pos = 0; pos < n && sc.state != ST_DONE; pos++) sc.byte<false>(table, row[ring_index(r, cap, pos)], pos, nullptr, 0);
    }
    if (sel) {
      removed[s] = sc.finish_streaming(&res[s], n);
      listed = sc.status != FSKHIP_XM_NEED_MORE || sc.packets + sc.dropped > 0u;
      data_len = sc.data_len;
    }
  }
  if (valid) flags[s] = sel ? (listed ? (kTouched | kListed) : kTouched) : 0u;
  const Pick P = pick_scan(listed, data_len, ws);
  if (threadIdx.x == 0u) pairs[blockIdx.x] = make_uint2(P.tot_s, P.tot_b);
}

__global__ __launch_bounds__(256) void xm_rx_commit_kernel(ProcState T, uint32_t n_streams, XmRxState X, const fskhip_xmodem_result *__restrict__ res,
                                                           const uint32_t *__restrict__ removed, const uint32_t *__restrict__ flags,
                                                           const uint2 *__restrict__ pairs, const uint32_t *__restrict__ totals,
                                                           uint32_t *__restrict__ streams, fskhip_xmodem_result *__restrict__ results,
                                                           uint32_t *__restrict__ offsets, uint8_t *__restrict__ data) {
  __shared__ uint32_t ws[4][2];
  __shared__ SpanJob jobs[4][64];
  if (totals[2] == 0u) return;   // a cap is too small: nothing is committed (the same word for every lane of the grid)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cap = T.rx_cap;
  const uint32_t f = s < n_streams ? flags[s] : 0u;
  const bool touched = (f & kTouched) != 0u, listed = (f & kListed) != 0u;
  fskhip_xmodem_result R{};
  if (touched) R = res[s];
  const Pick P = pick_scan(listed, R.data_len, ws);
  const uint2 base = pairs[blockIdx.x];
  if (blockIdx.x == 0u && threadIdx.x == 0u && offsets) offsets[totals[0]] = totals[1];
  uint32_t dst = base.y + P.pos_b;
  if (listed) {
    streams[base.x + P.pos_s] = s;
    offsets[base.x + P.pos_s] = dst;
    results[base.x + P.pos_s] = R;
  }
  const uint32_t r = touched ? T.rx_r[s] : 0u;
  const uint32_t held = touched ? T.rx_len[s] : 0u;
  const uint32_t e0 = touched ? X.expected[s] : 1u;
  // (header validity -- seq + nseq = 255, seq the expected sequence or the one before it -- is the scan pass's finding for every
  // packet inside R.consumed: this walk only tells an accepted packet, seq == e, from a duplicate, and checks nothing again)
  // the accepted payloads: one span per lane and round.  `left` bytes are still to be posted; the walk stays inside the span the
  // scan pass consumed, so a state it did not see ends the lane's rounds instead of running on
  {
    const uint8_t *row = T.rx_buf + (size_t)(touched ? s : 0u) * cap;
    const uint32_t end = R.consumed <= held ? R.consumed : held;
    uint32_t left = listed ? R.data_len : 0u, pos = 0u, e = e0;
    while (__builtin_amdgcn_ballot_w64(left > 0u) != 0ull) {   // (the same for every lane of the wave)
      SpanJob mine{0u, 0u, 0u, 0u};
      while (left > 0u && mine.len == 0u) {
        if (pos + 6u > end) { left = 0u; break; }
        if (row[ring_index(r, cap, pos)] != kSOH) { pos++; continue; }   // line noise between packets
        const uint32_t seq = row[ring_index(r, cap, pos + 1u)], len = row[ring_index(r, cap, pos + 3u)];
        if (pos + 6u + len > end) { left = 0u; break; }
        if (seq == e) {   // accepted (a duplicate carries the sequence before it and is stepped over)
          e = (e % 255u) + 1u;
          if (len > left) { left = 0u; break; }
          if (len) {
            mine = SpanJob{s, ring_index(r, cap, pos + 4u), len, dst};
            dst += len;
            left -= len;
          }
        }
        pos += 6u + len;
      }
      const bool have = mine.len != 0u;
      const uint64_t vote = __builtin_amdgcn_ballot_w64(have);
      const uint32_t n_jobs = (uint32_t)__builtin_popcountll(vote);
      if (have) jobs[wv][__builtin_popcountll(vote & ((1ull << lane) - 1ull))] = mine;
      const uint32_t longest = wave_max(mine.len);
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
            if (k < J[u].len) data[(size_t)J[u].dst + k] = v[u];
        }
      }
      wave_sync();   // (the jobs have been read before the next round posts its own)
    }
  }
  if (touched) {   // readIndex advanced by what left the ring, modulo the capacity; writeIndex and the bytes stay
    const uint32_t gone = removed[s] <= held ? removed[s] : held;
    T.rx_r[s] = ring_index(r, cap, gone);   // (a full ring taken out whole comes back to where it was)
    T.rx_len[s] = held - gone;
    X.expected[s] = R.expected_after;
    X.packets[s] += R.packets;
    X.dropped[s] += R.dropped;
  }
}

uint32_t groups_of(uint32_t n_streams) { return n_streams ? (n_streams + 255u) / 256u : 1u; }   // (an empty batch still writes its totals)

}  // namespace

size_t xmodem_rx_pair_words(uint32_t n_streams) { return 2u * (size_t)groups_of(n_streams); }

hipError_t launch_xmodem_rx_scan(const ProcState &T, uint32_t n_streams, const uint8_t *d_mask, const XmRxState &X, const XmRxScratch &W, uint32_t cap_streams,
                                 uint64_t cap_bytes, uint32_t *d_totals, hipStream_t st) {
  const uint32_t groups = groups_of(n_streams);
  if ((T.rx_cap & 15u) == 0u)
    hipLaunchKernelGGL(xm_rx_scan_kernel<true>, dim3(groups), dim3(256), 0, st, T, d_mask, n_streams, X.expected, W.res, W.removed, W.flags, (uint2 *)W.pairs);
  else
    hipLaunchKernelGGL(xm_rx_scan_kernel<false>, dim3(groups), dim3(256), 0, st, T, d_mask, n_streams, X.expected, W.res, W.removed, W.flags, (uint2 *)W.pairs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_drain_totals(W.pairs, groups, cap_streams, cap_bytes, d_totals, st);
}

hipError_t launch_xmodem_rx_commit(const ProcState &T, uint32_t n_streams, const XmRxState &X, const XmRxScratch &W, const uint32_t *d_totals, uint32_t *d_streams,
                                   fskhip_xmodem_result *d_results, uint32_t *d_offsets, uint8_t *d_data, hipStream_t st) {
  hipLaunchKernelGGL(xm_rx_commit_kernel, dim3(groups_of(n_streams)), dim3(256), 0, st, T, n_streams, X, W.res, W.removed, W.flags, (const uint2 *)W.pairs, d_totals,
                     d_streams, d_results, d_offsets, d_data);
  return hipGetLastError();
}

}  // namespace fsk
