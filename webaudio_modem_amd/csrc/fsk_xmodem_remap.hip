// fsk_xmodem_remap.hip -- the device half of fskhip_xmodem_{rx,tx,recv}_remap / _snapshot / _restore (include/fskhip_next.h): the
// per-stream words of a resident XModem handle gathered into another handle, packed into or taken out of an image's word table;
// and the files that go with them -- the sender's packed store, the file receiver's rows, an image's file area -- moved as a list
// of spans.
//
// Two kinds of data, two access shapes (as fsk_processor_remap.hip has them):
//   words  [stream] arrays of 4 bytes, at most eight per handle (XmWords).  One lane per destination stream: stores walk the
//          destination in its own order (coalesced), loads are gathers through the map, all of a stream's in flight together.  A
//          record of an image's table is 16 or 32 bytes and is read or written as quads.
//   spans  (src, dst, len) byte ranges of any length, 0 included, and any alignment at either end.  Sixteen lanes share a span and
//          a workgroup holds sixteen spans at once, so short files fill a wave; a span is cut into pieces of 4 KB and up to eight
//          workgroups (blockIdx.y) stride over the pieces of a long one.  Where source and destination agree modulo 16 a piece
//          goes as byte head, 16-byte quads (consecutive lanes on consecutive quads: 256 contiguous bytes per access, four
//          accesses loaded before the first store) and byte tail.  Where they agree only modulo 4: dwords.  Otherwise the
//          destination is still written in aligned dwords, each funnel-shifted out of the two aligned source dwords it straddles
//          (the last dword of such a piece goes bytewise, so no load reaches behind the span).  Spans write disjoint ranges: no
//          atomics.
// Only live bytes move: a span is a file's length, not its row, and an empty file costs its words.
//
// Offsets of a file receiver's snapshot are made here, its file_len being on the device: sum per workgroup, scan of the sums,
// scan within the workgroup (64-bit: a selection may name a stream many times).  The same passes find the longest file, which
// sizes the copy's grid: a row's capacity says nothing about what it holds.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "fsk_launch.h"

namespace fsk {

namespace {

constexpr uint32_t kPiece = 4096;    // bytes of a span one sub-group moves before it strides on (a multiple of 16)
constexpr uint32_t kSub = 16;        // lanes per span
constexpr uint32_t kInFlight = 4;    // accesses whose loads are issued before the first store

template <bool FROM_IMAGE>
__global__ __launch_bounds__(256) void xm_words_gather_kernel(XmWords D, uint32_t n_dst, const int64_t *__restrict__ map, XmWords S,
                                                              const uint32_t *__restrict__ table, uint32_t record_words) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_dst; i += gridDim.x * 256u) {
    const int64_t m = map[i];
    uint32_t w[8];
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) w[k] = D.fresh[k];
    if (m >= 0) {
      if (FROM_IMAGE) {   // (records are 16 or 32 bytes, the table is 16-byte aligned)
        const uint4 *r = (const uint4 *)(table + (size_t)m * record_words);
        const uint4 q0 = r[0];
        w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w;
        if (record_words > 4u) {
          const uint4 q1 = r[1];
          w[4] = q1.x; w[5] = q1.y; w[6] = q1.z; w[7] = q1.w;
        }
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++)
          if (k < D.n) w[k] = S.a[k][m];
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++)
      if (k < D.n) D.a[k][i] = w[k];
  }
}

__global__ __launch_bounds__(256) void xm_words_pack_kernel(XmWords S, const int64_t *__restrict__ sel, uint32_t n, uint32_t record_words, uint32_t flag7,
                                                            uint32_t *__restrict__ table) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n; r += gridDim.x * 256u) {
    const size_t s = sel ? (size_t)sel[r] : r;   // (the host checked sel against the batch)
    uint32_t w[8];
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) w[k] = k < S.n ? S.a[k][s] : 0u;
    if (flag7) w[7] = w[7] != 0u ? 1u : 0u;
    uint4 *o = (uint4 *)(table + (size_t)r * record_words);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    if (record_words > 4u) o[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

// n bytes from s to d by the sixteen lanes l = 0..15 of a sub-group
__device__ __forceinline__ void copy_piece(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, uint32_t n, uint32_t l) {
  const uint32_t sa = (uint32_t)(uintptr_t)s, da = (uint32_t)(uintptr_t)d;
  if (((sa ^ da) & 15u) == 0u) {
    const uint32_t head = min(n, (16u - (da & 15u)) & 15u);
    if (l < head) d[l] = s[l];
    const uint32_t nq = (n - head) >> 4;
    const uint4 *sq = (const uint4 *)(s + head);
    uint4 *dq = (uint4 *)(d + head);
    for (uint32_t q = l; q < nq; q += kSub * kInFlight) {
      uint4 v[kInFlight];
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++)
        if (q + u * kSub < nq) v[u] = sq[q + u * kSub];
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++)
        if (q + u * kSub < nq) dq[q + u * kSub] = v[u];
    }
    const uint32_t done = head + (nq << 4);
    if (l < n - done) d[done + l] = s[done + l];
    return;
  }
  const uint32_t head = min(n, (4u - (da & 3u)) & 3u);
  if (l < head) d[l] = s[l];
  const uint32_t r = (sa + head) & 3u;
  uint32_t nw = (n - head) >> 2;
  uint32_t *dw = (uint32_t *)(d + head);
  if (r == 0u) {
    const uint32_t *sw = (const uint32_t *)(s + head);
    for (uint32_t q = l; q < nw; q += kSub * kInFlight) {
      uint32_t v[kInFlight];
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++)
        if (q + u * kSub < nw) v[u] = sw[q + u * kSub];
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++)
        if (q + u * kSub < nw) dw[q + u * kSub] = v[u];
    }
  } else {
    // dword q of the destination is source bytes [r + 4q, r + 4q + 4) counted from sw = s + head - r: the upper 4 - r bytes of the
    // aligned dword q and the lower r bytes of dword q + 1.  sw lies inside the source's allocation (whose base is dword-aligned);
    // the last dword's second load would reach up to 3 bytes behind the span, so that dword is left to the byte tail.
    if (nw) nw -= 1u;
    const uint32_t *sw = (const uint32_t *)(s + head - r);
    const uint32_t sh = r * 8u;
    for (uint32_t q = l; q < nw; q += kSub * kInFlight) {
      uint32_t lo[kInFlight], hi[kInFlight];
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++)
        if (q + u * kSub < nw) { lo[u] = sw[q + u * kSub]; hi[u] = sw[q + u * kSub + 1u]; }
#pragma unroll
      for (uint32_t u = 0; u < kInFlight; u++)
        if (q + u * kSub < nw) dw[q + u * kSub] = (lo[u] >> sh) | (hi[u] << (32u - sh));
    }
  }
  const uint32_t done = head + (nw << 2);   // (fewer than 8 bytes are left)
  if (l < n - done) d[done + l] = s[done + l];
}

__global__ __launch_bounds__(256) void xm_span_copy_kernel(const uint8_t *__restrict__ sbase, uint8_t *__restrict__ dbase, const XmSpan *__restrict__ spans,
                                                           uint32_t n_spans) {
  const uint32_t l = threadIdx.x & (kSub - 1u), sub = threadIdx.x / kSub;
  for (uint64_t j = (uint64_t)blockIdx.x * (256u / kSub) + sub; j < n_spans; j += (uint64_t)gridDim.x * (256u / kSub)) {
    const XmSpan J = spans[j];
    for (uint64_t p = (uint64_t)blockIdx.y * kPiece; p < J.len; p += (uint64_t)gridDim.y * kPiece)
      copy_piece(sbase + J.src + p, dbase + J.dst + p, (uint32_t)min((uint64_t)kPiece, J.len - p), l);
  }
}

__global__ __launch_bounds__(256) void xm_recv_plan_kernel(const uint32_t *__restrict__ src_len, uint32_t src_cap, uint32_t dst_cap, const int64_t *__restrict__ map,
                                                           uint32_t n_dst, XmSpan *__restrict__ spans, uint32_t *__restrict__ bad) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_dst; i += gridDim.x * 256u) {
    const int64_t m = map[i];
    const uint32_t len = m >= 0 ? src_len[m] : 0u;
    if (len > dst_cap) atomicMin(bad, i);
    if (len) atomicMax(bad + 1, len);
    spans[i] = XmSpan{m >= 0 ? (uint64_t)m * src_cap : 0u, (uint64_t)i * dst_cap, len};
  }
}

__device__ __forceinline__ uint32_t sel_len(const uint32_t *__restrict__ len, const int64_t *__restrict__ sel, uint32_t r, uint32_t n) {
  return r < n ? len[sel ? (size_t)sel[r] : r] : 0u;
}

// inclusive scan of one value per thread over the workgroup (through LDS: these kernels are not on a hot path)
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t *sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = 1u; o < 256u; o <<= 1) {
    const uint64_t add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
    __syncthreads();
    sh[threadIdx.x] += add;
    __syncthreads();
  }
  return sh[threadIdx.x];
}

__global__ __launch_bounds__(256) void xm_len_sums_kernel(const uint32_t *__restrict__ len, const int64_t *__restrict__ sel, uint32_t n, uint64_t *__restrict__ sums) {
  __shared__ uint64_t sh[256];
  const uint32_t v = sel_len(len, sel, blockIdx.x * 256u + threadIdx.x, n);
  const uint64_t inc = block_scan(v, sh);
  if (threadIdx.x == 255u) sums[blockIdx.x] = inc;
  if (v) atomicMax((unsigned long long *)(sums + gridDim.x + 1u), (unsigned long long)v);   // the longest file, behind the total
}

// sums[0 .. n_groups): each workgroup's bytes -> the bytes of the workgroups before it; sums[n_groups] = all of them
__global__ __launch_bounds__(256) void xm_sums_scan_kernel(uint64_t *__restrict__ sums, uint32_t n_groups) {
  __shared__ uint64_t sh[256];
  uint64_t carry = 0u;
  for (uint32_t base = 0; base < n_groups; base += 256u) {   // (the same trip count in every lane: barriers in block_scan)
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < n_groups ? sums[i] : 0u;
    const uint64_t inc = block_scan(v, sh);
    if (i < n_groups) sums[i] = carry + inc - v;
    carry += sh[255];
    __syncthreads();
  }
  if (threadIdx.x == 0u) sums[n_groups] = carry;
}

__global__ __launch_bounds__(256) void xm_offsets_kernel(const uint32_t *__restrict__ len, const int64_t *__restrict__ sel, uint32_t n, const uint64_t *__restrict__ sums,
                                                         uint64_t *__restrict__ offsets) {
  __shared__ uint64_t sh[256];
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  const uint32_t v = sel_len(len, sel, r, n);
  const uint64_t inc = block_scan(v, sh);
  if (r < n) offsets[r] = sums[blockIdx.x] + inc - v;
  if (r == n - 1u) offsets[n] = sums[blockIdx.x] + inc;
}

__global__ __launch_bounds__(256) void xm_recv_spans_kernel(const uint32_t *__restrict__ len, uint32_t cap, const int64_t *__restrict__ sel, uint32_t n,
                                                            const uint64_t *__restrict__ offsets, XmSpan *__restrict__ spans) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n; r += gridDim.x * 256u) {
    const uint64_t s = sel ? (uint64_t)sel[r] : r;
    spans[r] = XmSpan{s * cap, offsets[r], len[s]};
  }
}

uint32_t grid_for(uint32_t n) { return min((n + 255u) / 256u, 2048u); }
uint32_t groups_of(uint32_t n) { return (n + 255u) / 256u; }

}  // namespace

hipError_t launch_xmodem_words_gather(const XmWords &D, uint32_t n_dst, const int64_t *d_map, const XmWords *S, const uint32_t *d_table, uint32_t record_words,
                                      hipStream_t st) {
  if (n_dst == 0) return hipSuccess;
  if (S)
    hipLaunchKernelGGL(xm_words_gather_kernel<false>, dim3(grid_for(n_dst)), dim3(256), 0, st, D, n_dst, d_map, *S, nullptr, 0u);
  else
    hipLaunchKernelGGL(xm_words_gather_kernel<true>, dim3(grid_for(n_dst)), dim3(256), 0, st, D, n_dst, d_map, XmWords{}, d_table, record_words);
  return hipGetLastError();
}

hipError_t launch_xmodem_words_pack(const XmWords &S, const int64_t *d_sel, uint32_t n, uint32_t record_words, bool flag7, uint32_t *d_table, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(xm_words_pack_kernel, dim3(grid_for(n)), dim3(256), 0, st, S, d_sel, n, record_words, flag7 ? 1u : 0u, d_table);
  return hipGetLastError();
}

hipError_t launch_xmodem_span_copy(const uint8_t *d_src, uint8_t *d_dst, const XmSpan *d_spans, uint32_t n_spans, uint64_t max_len, hipStream_t st) {
  if (n_spans == 0 || max_len == 0) return hipSuccess;
  const uint32_t gx = min((n_spans + 15u) / 16u, 2048u), gy = (uint32_t)std::min<uint64_t>((max_len + kPiece - 1u) / kPiece, 8u);
  hipLaunchKernelGGL(xm_span_copy_kernel, dim3(gx, gy), dim3(256), 0, st, d_src, d_dst, d_spans, n_spans);
  return hipGetLastError();
}

hipError_t launch_xmodem_recv_plan(const uint32_t *d_src_len, uint32_t src_cap, uint32_t dst_cap, const int64_t *d_map, uint32_t n_dst, XmSpan *d_spans,
                                   uint32_t *d_bad, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d_bad, 0xFF, sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(d_bad + 1, 0, sizeof(uint32_t), st);
  if (e != hipSuccess || n_dst == 0) return e;
  hipLaunchKernelGGL(xm_recv_plan_kernel, dim3(grid_for(n_dst)), dim3(256), 0, st, d_src_len, src_cap, dst_cap, d_map, n_dst, d_spans, d_bad);
  return hipGetLastError();
}

size_t xmodem_offsets_scratch_words(uint32_t n) { return (size_t)groups_of(n) + 2u; }

hipError_t launch_xmodem_file_offsets(const uint32_t *d_len, const int64_t *d_sel, uint32_t n, uint64_t *d_offsets, uint64_t *d_sums, hipStream_t st) {
  const uint32_t groups = groups_of(n);
  hipError_t e = hipMemsetAsync(d_sums + groups, 0, 2u * sizeof(uint64_t), st);   // the total and the longest file
  if (e != hipSuccess) return e;
  if (n == 0) return hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), st);
  hipLaunchKernelGGL(xm_len_sums_kernel, dim3(groups), dim3(256), 0, st, d_len, d_sel, n, d_sums);
  hipLaunchKernelGGL(xm_sums_scan_kernel, dim3(1), dim3(256), 0, st, d_sums, groups);
  hipLaunchKernelGGL(xm_offsets_kernel, dim3(groups), dim3(256), 0, st, d_len, d_sel, n, d_sums, d_offsets);
  return hipGetLastError();
}

hipError_t launch_xmodem_recv_spans(const uint32_t *d_len, uint32_t cap, const int64_t *d_sel, uint32_t n, const uint64_t *d_offsets, XmSpan *d_spans,
                                    hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(xm_recv_spans_kernel, dim3(grid_for(n)), dim3(256), 0, st, d_len, cap, d_sel, n, d_offsets, d_spans);
  return hipGetLastError();
}

}  // namespace fsk
