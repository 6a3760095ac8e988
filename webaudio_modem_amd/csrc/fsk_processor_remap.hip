// fsk_processor_remap.hip -- the device half of fskhip_processor_remap / _snapshot / _restore (include/fskhip_next.h): a
// stream's FSKProcessor state -- the RX byte ring with its three words, the pending modulation's generator words, phase and
// payload, the `completed` count (fsk_params.h ProcState) -- gathered into another processor, or packed into / taken out of
// stream-major records (ProcImage).
//
// Two kinds of data, two access shapes:
//   words  [stream] arrays of 4 (phase: 8) bytes.  One lane per destination stream: stores walk the destination in its own
//          order (coalesced), loads are gathers through the map that coalesce wherever it has runs, thirteen of them in flight.
//   rows   rx_buf [stream][rx_cap] and tx_payload [stream][pitch], stream-major.  Moved in 16-byte quads, consecutive lanes on
//          consecutive quads of ONE row (lanes-per-row = the row's quads rounded up to a power of two, at most 64: a 1 KB ring is
//          one wave-wide access, a 48-byte one shares the wave with 15 others), so every access is a contiguous run.
// Only what is live moves.  A wave takes 64 streams, reads their words, and lists the rows that hold anything -- a ring with
// _length > 0, a payload behind a live signal -- compacted through LDS; the quads of a listed row that lie outside its live span
// [readIndex, readIndex + _length) (wrap included, rounded out to quads) are skipped too.  A drained ring costs its three words.
// Four rows (or four sets of rows) per wave are loaded before any is stored.  The grid is sized to the device, not to the batch:
// workgroups stride over the groups of 64 streams, so 262 144 streams keep every CU at seven waves per SIMD (49 VGPRs, no scratch) until the end.
//
// Rings whose capacity is not a multiple of 16 have unaligned rows: those go byte by byte (same spans, same result).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_launch.h"
#include "fsk_params.h"

namespace fsk {

namespace {

constexpr uint32_t kInFlight = 4;   // row passes whose loads are issued before the first store

struct RowJob { uint32_t src, dst, start, len; };   // a row with a live span: bytes [start, start + len) of src's row, modulo the capacity

// the words of one stream, in the order of a record's fixed part (fsk_params.h ProcImage)
struct ProcWords {
  uint32_t w[12];
  double phase;
};

__device__ __forceinline__ ProcWords load_words(const ProcState &T, uint32_t s) {
  ProcWords W;
  W.w[0] = T.rx_w[s]; W.w[1] = T.rx_r[s]; W.w[2] = T.rx_len[s];
  W.w[3] = T.tx_pending[s]; W.w[4] = T.tx_completed[s]; W.w[5] = T.tx_pos[s]; W.w[6] = T.tx_len[s]; W.w[7] = T.tx_n_payload[s];
  W.w[8] = T.tx_in_bit[s]; W.w[9] = T.tx_bit_idx[s]; W.w[10] = T.tx_cur_bit[s]; W.w[11] = 0u;
  W.phase = T.tx_phase[s];
  return W;
}
__device__ __forceinline__ void store_words(const ProcState &T, uint32_t s, const ProcWords &W) {
  T.rx_w[s] = W.w[0]; T.rx_r[s] = W.w[1]; T.rx_len[s] = W.w[2];
  T.tx_pending[s] = W.w[3]; T.tx_completed[s] = W.w[4]; T.tx_pos[s] = W.w[5]; T.tx_len[s] = W.w[6]; T.tx_n_payload[s] = W.w[7];
  T.tx_in_bit[s] = W.w[8]; T.tx_bit_idx[s] = W.w[9]; T.tx_cur_bit[s] = W.w[10];
  T.tx_phase[s] = W.phase;
}
__device__ __forceinline__ bool signal_live(const ProcWords &W) { return W.w[3] != 0u && W.w[6] != 0u; }   // pending, and a signal to feed

// does byte x of a row of `cap` bytes lie in [start, start + len) modulo cap?
__device__ __forceinline__ bool byte_live(uint32_t x, uint32_t start, uint32_t len, uint32_t cap) {
  if (x >= cap) return false;
  const uint32_t d = x >= start ? x - start : x + cap - start;
  return d < len;
}
// does the quad at byte a = 16k hold any live byte?
__device__ __forceinline__ bool quad_live(uint32_t a, uint32_t start, uint32_t len, uint32_t cap) {
  const uint32_t b = min(a + 16u, cap), e = start + len;
  return len != 0u && ((a < min(e, cap) && b > start) || (e > cap && a < e - cap));
}

// 16 bytes at p, of which `lim` exist (the row ends there); aligned rows in one access
__device__ __forceinline__ uint4 ld16(const uint8_t *p, uint32_t lim, bool aligned) {
  if (aligned && lim >= 16u) return *(const uint4 *)p;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  for (uint32_t b = 0; b < 16u && b < lim; b++) w[b >> 2] |= (uint32_t)p[b] << (8u * (b & 3u));
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void st16(uint8_t *p, uint4 v, uint32_t lim, bool aligned) {
  if (aligned && lim >= 16u) { *(uint4 *)p = v; return; }
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  for (uint32_t b = 0; b < 16u && b < lim; b++) p[b] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
}

__device__ __forceinline__ uint32_t lanes_per_row(uint32_t quads) {
  uint32_t l = 1u;
  while (l < quads && l < 64u) l <<= 1;
  return l;
}

// The live quads of n_jobs rows: row J.src of the source to row J.dst of the destination.  `cap` is the row's capacity (where a
// span wraps, where a row ends); s_lim / d_lim the bytes a source / destination row really has (a record's ring is padded to quads).
__device__ __forceinline__ void move_rows(const RowJob *jobs, uint32_t n_jobs, uint32_t lane, const uint8_t *__restrict__ sbase, size_t spitch, uint32_t s_lim,
                                          bool s_aligned, uint8_t *__restrict__ dbase, size_t dpitch, uint32_t d_lim, bool d_aligned, uint32_t cap) {
  const uint32_t quads = (cap + 15u) >> 4, lpr = lanes_per_row(quads), rpp = 64u / lpr;
  const uint32_t sub = lane / lpr, k0 = lane % lpr;
  for (uint32_t p = 0; p < n_jobs; p += rpp * kInFlight) {
    for (uint32_t kb = 0; kb < quads; kb += lpr) {
      const uint32_t a = (kb + k0) << 4;
      uint4 v[kInFlight];
      uint32_t drow[kInFlight];
      bool on[kInFlight];
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++) {
        const uint32_t slot = p + u * rpp + sub;
        on[u] = false;
        if (slot < n_jobs && kb + k0 < quads) {
          const RowJob J = jobs[slot];
          on[u] = quad_live(a, J.start, J.len, cap);
          drow[u] = J.dst;
          if (on[u]) v[u] = ld16(sbase + (size_t)J.src * spitch + a, s_lim - a, s_aligned);
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++)
        if (on[u]) st16(dbase + (size_t)drow[u] * dpitch + a, v[u], d_lim - a, d_aligned);
    }
  }
}

// Compacts the lanes with `live` into jobs[0 .. n): returns n (the same in every lane of the wave)
__device__ __forceinline__ uint32_t list_rows(RowJob *jobs, bool live, const RowJob &J, uint32_t lane) {
  const uint64_t mask = __builtin_amdgcn_ballot_w64(live);
  if (live) jobs[__builtin_popcountll(mask & ((1ull << lane) - 1ull))] = J;
  return (uint32_t)__builtin_popcountll(mask);
}

// Stream i of D continues stream map[i] of S (FROM_IMAGE: record map[i] of the image, where the slab I holds it), or starts as
// fskhip_processor_create leaves a stream where map[i] = -1 (FROM_IMAGE: only in the launch that has fresh_too).
template <bool FROM_IMAGE>
__global__ __launch_bounds__(256) void proc_gather_kernel(ProcState D, uint32_t n_dst, const int64_t *__restrict__ map, ProcState S, ProcImage I, uint32_t fresh_too) {
  __shared__ RowJob jobs[4][2][64];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t n_groups = (n_dst + 63u) >> 6;
  const uint32_t cap = D.rx_cap;
  const bool ring_aligned = (cap & 15u) == 0u;
  for (uint32_t g0 = blockIdx.x * 4u; g0 < n_groups; g0 += gridDim.x * 4u) {   // (the same trip count for the four waves: barriers below)
    const uint32_t i = (g0 + wv) * 64u + lane;
    const int64_t mi = i < n_dst ? map[i] : -2;
    const bool cont = FROM_IMAGE ? (mi >= (int64_t)I.first && mi < (int64_t)I.first + (int64_t)I.count) : mi >= 0;
    const bool fresh = mi == -1 && (!FROM_IMAGE || fresh_too != 0u);
    const uint32_t m = cont ? (uint32_t)(FROM_IMAGE ? mi - (int64_t)I.first : mi) : 0u;
    ProcWords W{};
    if (cont) {
      if (FROM_IMAGE) {
        const uint4 *r = (const uint4 *)(I.rec + (size_t)m * I.rec_bytes);
        const uint4 q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3];
        W.w[0] = q0.x; W.w[1] = q0.y; W.w[2] = q0.z; W.w[3] = q0.w; W.w[4] = q1.x; W.w[5] = q1.y; W.w[6] = q1.z; W.w[7] = q1.w;
        W.w[8] = q2.x; W.w[9] = q2.y; W.w[10] = q2.z;
        W.phase = __builtin_bit_cast(double, (uint64_t)q3.x | ((uint64_t)q3.y << 32));
      } else {
        W = load_words(S, m);
      }
    }
    if (cont || fresh) store_words(D, i, W);
    const bool ring = cont && W.w[2] != 0u, pay = cont && signal_live(W) && W.w[7] != 0u;
    const uint32_t n_ring = list_rows(jobs[wv][0], ring, RowJob{m, i, W.w[1], W.w[2]}, lane);
    const uint32_t n_pay = list_rows(jobs[wv][1], pay, RowJob{m, i, 0u, W.w[7]}, lane);
    __syncthreads();
    if (FROM_IMAGE) {
      move_rows(jobs[wv][0], n_ring, lane, I.rec + kProcRecFixed + I.pay_cap, I.rec_bytes, I.ring_pitch, true, D.rx_buf, cap, cap, ring_aligned, cap);
      move_rows(jobs[wv][1], n_pay, lane, I.rec + kProcRecFixed, I.rec_bytes, I.pay_cap, true, D.tx_payload, D.tx_payload_pitch, (uint32_t)D.tx_payload_pitch, true,
                min(I.pay_cap, (uint32_t)D.tx_payload_pitch));
    } else {
      move_rows(jobs[wv][0], n_ring, lane, S.rx_buf, cap, cap, ring_aligned, D.rx_buf, cap, cap, ring_aligned, cap);
      move_rows(jobs[wv][1], n_pay, lane, S.tx_payload, S.tx_payload_pitch, (uint32_t)S.tx_payload_pitch, true, D.tx_payload, D.tx_payload_pitch,
                (uint32_t)D.tx_payload_pitch, true, (uint32_t)min(S.tx_payload_pitch, D.tx_payload_pitch));
    }
    __syncthreads();
  }
}

// Records [0, count) of the slab I = streams sel[I.first ..] of S (sel null: I.first, I.first + 1, ...), in canonical form: every
// byte of a record is written, and is zero unless it is a word, a pending payload's byte or a ring byte inside the live span.
__global__ __launch_bounds__(256) void proc_pack_kernel(ProcState S, const int64_t *__restrict__ sel, ProcImage I, uint8_t *__restrict__ out) {
  __shared__ RowJob jobs[4][64];
  __shared__ uint32_t npay[4][64];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t n_groups = (I.count + 63u) >> 6;
  const uint32_t cap = S.rx_cap;
  const bool ring_aligned = (cap & 15u) == 0u;
  const uint32_t pq = I.pay_cap >> 4, quads = pq + (I.ring_pitch >> 4), lpr = lanes_per_row(quads), rpp = 64u / lpr;
  const uint32_t sub = lane / lpr, k0 = lane % lpr;
  for (uint32_t g0 = blockIdx.x * 4u; g0 < n_groups; g0 += gridDim.x * 4u) {
    const uint32_t r0 = (g0 + wv) * 64u, r = r0 + lane;
    const uint32_t n_rows = r0 < I.count ? min(64u, I.count - r0) : 0u;
    if (r < I.count) {
      const uint32_t s = sel ? (uint32_t)sel[(size_t)I.first + r] : I.first + r;   // (the host checked sel against the batch)
      ProcWords W = load_words(S, s);
      const bool sig = signal_live(W);
      W.w[3] = W.w[3] != 0u ? 1u : 0u;
      if (!sig) { W.w[5] = 0u; W.w[6] = 0u; W.w[7] = 0u; W.w[8] = 0u; W.w[9] = 0u; W.w[10] = 0u; W.phase = 0.0; }
      const uint64_t ph = __builtin_bit_cast(uint64_t, W.phase);
      uint4 *o = (uint4 *)(out + (size_t)r * I.rec_bytes);
      o[0] = make_uint4(W.w[0], W.w[1], W.w[2], W.w[3]);
      o[1] = make_uint4(W.w[4], W.w[5], W.w[6], W.w[7]);
      o[2] = make_uint4(W.w[8], W.w[9], W.w[10], 0u);
      o[3] = make_uint4((uint32_t)ph, (uint32_t)(ph >> 32), 0u, 0u);
      jobs[wv][lane] = RowJob{s, r, W.w[1], W.w[2]};
      npay[wv][lane] = W.w[7];
    }
    __syncthreads();
    for (uint32_t p = 0; p < n_rows; p += rpp) {
      const uint32_t slot = p + sub;
      if (slot >= n_rows) continue;
      const RowJob J = jobs[wv][slot];
      const uint32_t np = npay[wv][slot];
      for (uint32_t k = k0; k < quads; k += lpr) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        uint32_t keep[4] = {0u, 0u, 0u, 0u};
        if (k < pq) {   // payload quad: bytes [0, np) are the pending payload
          const uint32_t a = k << 4;
          if (a < np) {
            v = ld16(S.tx_payload + (size_t)J.src * S.tx_payload_pitch + a, (uint32_t)S.tx_payload_pitch - a, true);
#pragma unroll
            for (uint32_t b = 0; b < 16u; b++)
              if (a + b < np) keep[b >> 2] |= 0xFFu << (8u * (b & 3u));
          }
        } else {        // ring quad
          const uint32_t a = (k - pq) << 4;
          if (a < cap && quad_live(a, J.start, J.len, cap)) {
            v = ld16(S.rx_buf + (size_t)J.src * cap + a, cap - a, ring_aligned);
#pragma unroll
            for (uint32_t b = 0; b < 16u; b++)
              if (byte_live(a + b, J.start, J.len, cap)) keep[b >> 2] |= 0xFFu << (8u * (b & 3u));
          }
        }
        v.x &= keep[0]; v.y &= keep[1]; v.z &= keep[2]; v.w &= keep[3];
        *(uint4 *)(out + (size_t)J.dst * I.rec_bytes + kProcRecFixed + ((size_t)k << 4)) = v;
      }
    }
    __syncthreads();
  }
}

// out[0] = the longest pending payload (bytes) among the streams idx[0 .. n) of S (idx null: streams 0 .. n - 1; entries < 0 skipped)
__global__ __launch_bounds__(256) void proc_max_payload_kernel(ProcState S, const int64_t *__restrict__ idx, uint32_t n, uint32_t *__restrict__ out) {
  uint32_t best = 0u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const int64_t m = idx ? idx[i] : (int64_t)i;
    if (m < 0) continue;
    if (S.tx_pending[m] != 0u && S.tx_len[m] != 0u) best = max(best, S.tx_n_payload[m]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
  if ((threadIdx.x & 63u) == 0u && best != 0u) atomicMax(out, best);
}

// workgroups of four waves, 64 streams to a wave; at most 2 048 of them (eight to each of 256 CUs): larger batches stride
uint32_t grid_for(uint32_t n_streams) { return min((n_streams + 255u) / 256u, 2048u); }

}  // namespace

hipError_t launch_processor_gather(const ProcState &D, uint32_t n_dst, const int64_t *d_map, const ProcState &S, hipStream_t st) {
  if (n_dst == 0) return hipSuccess;
  hipLaunchKernelGGL(proc_gather_kernel<false>, dim3(grid_for(n_dst)), dim3(256), 0, st, D, n_dst, d_map, S, ProcImage{}, 0u);
  return hipGetLastError();
}

hipError_t launch_processor_unpack(const ProcState &D, uint32_t n_dst, const int64_t *d_map, const ProcImage &I, bool fresh_too, hipStream_t st) {
  if (n_dst == 0) return hipSuccess;
  hipLaunchKernelGGL(proc_gather_kernel<true>, dim3(grid_for(n_dst)), dim3(256), 0, st, D, n_dst, d_map, ProcState{}, I, fresh_too ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_processor_pack(const ProcState &S, const int64_t *d_sel, const ProcImage &I, void *d_out, hipStream_t st) {
  if (I.count == 0) return hipSuccess;
  hipLaunchKernelGGL(proc_pack_kernel, dim3(grid_for(I.count)), dim3(256), 0, st, S, d_sel, I, (uint8_t *)d_out);
  return hipGetLastError();
}

hipError_t launch_processor_max_payload(const ProcState &S, const int64_t *d_idx, uint32_t n, uint32_t *d_out, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d_out, 0, sizeof(uint32_t), st);
  if (e != hipSuccess || n == 0) return e;
  hipLaunchKernelGGL(proc_max_payload_kernel, dim3(min((n + 255u) / 256u, 1024u)), dim3(256), 0, st, S, d_idx, n, d_out);
  return hipGetLastError();
}

}  // namespace fsk
