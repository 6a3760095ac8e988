// fsk_snapshot.hip -- the device half of fskhip_snapshot_streams / fskhip_restore_streams (include/fskhip.h): a stream's whole
// state between its field-major home (fsk_params.h: [field][stream] RF_* / IF_* rows, [block][d][64] polyphase registers,
// [quad][stream] amplitude-ring quads) and ONE contiguous record (SnapLayout: ~1 KB, stream-major), so that the host can
// select, reorder and concatenate streams with memcpy.
//
// That is a transpose of ~250 words per stream.  A lane-per-stream loop like remap_kernel's would touch the records at a
// ~1 KB stride, so both kernels stage through LDS: a workgroup (four waves) takes 64 streams and walks their records in chunks
// of kSnapChunk words.
//   field side   lane = stream: every element (a 4-, 8- or 16-byte word of one field) is ONE 64-lane access, coalesced in the
//                engine's own stream order (pack: a gather through `sel`, coalescing where it has runs, as remap's loads do);
//   record side  consecutive lanes take consecutive 16-byte quads of a record: a chunk is 512 contiguous bytes per record.
// LDS tile [64][kSnapPitch] words.  The pitch is odd, so the field side's ds_write_b32 / ds_read_b32 (bank = word mod 32,
// conflicts within a 32-lane half) hit 32 banks; on the record side lane k of a row moves the four words of quad k, a stride
// of 4 words = 8 banks, 4-way -- so lane k starts its quad at word (k / 8) mod 4 and the eight lanes that shared a bank
// spread over four.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_launch.h"
#include "fsk_newstream.h"
#include "fsk_params.h"

namespace fsk {

static constexpr uint32_t kSnapChunk = 128;              // words of a record per LDS pass (a multiple of 4)
static constexpr uint32_t kSnapPitch = kSnapChunk + 1;   // odd

namespace {

// element `e` of a section for stream s, in elements of the section's own size
__device__ __forceinline__ size_t snap_elem(const SnapSection &sc, uint32_t e, uint32_t s, size_t n_streams, uint32_t d) {
  if (sc.kind == SNAP_POLY || sc.kind == SNAP_POLYU) return ((size_t)(s >> 6) * d + e) * 64u + (s & 63u);
  return (size_t)e * n_streams + s;
}
__device__ __forceinline__ void *snap_base(const DemodState &S, uint32_t kind) {
  return kind == SNAP_RF ? S.rs : kind == SNAP_IF ? (void *)S.is : kind == SNAP_POLY ? S.poly : kind == SNAP_POLYU ? S.poly_u : (void *)S.amp_ring;
}
// quad k of a row: four LDS words, taken in the order that starts at word (k / 8) mod 4 (see the file comment)
__device__ __forceinline__ uint4 tile_read_quad(const uint32_t *row, uint32_t k) {
  const uint32_t rot = (k >> 3) & 3u;
  uint32_t t[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) t[j] = row[4u * k + ((j + rot) & 3u)];   // t[j] = word (j + rot) & 3
  uint4 v;
  v.x = rot == 0 ? t[0] : rot == 1 ? t[3] : rot == 2 ? t[2] : t[1];
  v.y = rot == 0 ? t[1] : rot == 1 ? t[0] : rot == 2 ? t[3] : t[2];
  v.z = rot == 0 ? t[2] : rot == 1 ? t[1] : rot == 2 ? t[0] : t[3];
  v.w = rot == 0 ? t[3] : rot == 1 ? t[2] : rot == 2 ? t[1] : t[0];
  return v;
}
__device__ __forceinline__ void tile_write_quad(uint32_t *row, uint32_t k, uint4 v) {
  const uint32_t rot = (k >> 3) & 3u;
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t c = (j + rot) & 3u;
    row[4u * k + c] = c == 0 ? w[0] : c == 1 ? w[1] : c == 2 ? w[2] : w[3];
  }
}

__global__ __launch_bounds__(256) void snap_pack_kernel(SnapLayout L, DemodState S, uint32_t n_src, const int64_t *__restrict__ sel, uint32_t first,
                                                        uint32_t count, uint32_t *__restrict__ out) {
  __shared__ uint32_t tile[64 * kSnapPitch];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t r0 = blockIdx.x * 64u;
  const bool live = r0 + lane < count;
  const uint32_t s = live ? (sel ? (uint32_t)sel[(size_t)first + r0 + lane] : first + r0 + lane) : 0u;   // (the host checked sel against n_src)
  uint32_t *const mine = tile + lane * kSnapPitch;
  for (uint32_t c0 = 0; c0 < L.rec_words; c0 += kSnapChunk) {
    const uint32_t c1 = min(c0 + kSnapChunk, L.rec_words);
    for (uint32_t k = 0; k < L.n_sec; k++) {
      const SnapSection sc = L.sec[k];
      const uint32_t lo = max(sc.w0, c0), hi = min(sc.w0 + sc.n * sc.e, c1);
      if (lo >= hi) continue;
      const void *base = snap_base(S, sc.kind);
      const bool load = live && sc.kind != SNAP_ZERO;
      for (uint32_t e = (lo - sc.w0) / sc.e + wv; e < (hi - sc.w0) / sc.e; e += 4u) {
        uint32_t *t = mine + (sc.w0 + e * sc.e - c0);
        const size_t at = snap_elem(sc, e, s, n_src, L.d);
        if (sc.e == 1) {
          t[0] = load ? ((const uint32_t *)base)[at] : 0u;
        } else if (sc.e == 2) {
          const uint2 z = {0u, 0u};
          const uint2 v = load ? ((const uint2 *)base)[at] : z;
          t[0] = v.x; t[1] = v.y;
        } else {
          const uint4 z = {0u, 0u, 0u, 0u};
          const uint4 v = load ? ((const uint4 *)base)[at] : z;
          t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
      }
    }
    __syncthreads();
    const uint32_t nq = (c1 - c0) >> 2;
    for (uint32_t idx = threadIdx.x; idx < 64u * nq; idx += 256u) {
      const uint32_t rr = idx / nq, k = idx - rr * nq;
      if (r0 + rr < count) *(uint4 *)(out + (size_t)(r0 + rr) * L.rec_words + c0 + 4u * k) = tile_read_quad(tile + rr * kSnapPitch, k);
    }
    __syncthreads();
  }
}

template <typename Real>
__global__ __launch_bounds__(256) void snap_unpack_kernel(SnapLayout L, DemodState D, uint32_t n_dst, const int64_t *__restrict__ map, uint32_t rec_first,
                                                          uint32_t rec_count, uint32_t fresh_too, NewStream N, const uint32_t *__restrict__ in) {
  __shared__ uint32_t tile[64 * kSnapPitch];
  __shared__ int32_t srec[64];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * 64u + lane;
  const int64_t mi = i < n_dst ? map[i] : -2;
  const bool cont = mi >= (int64_t)rec_first && mi < (int64_t)rec_first + (int64_t)rec_count;
  const bool act = cont || (mi == -1 && fresh_too);
  if (!__syncthreads_or(act ? 1 : 0)) return;     // no stream of this group is served by this slab of records
  if (wv == 0) srec[lane] = cont ? (int32_t)(mi - (int64_t)rec_first) : -1;
  const uint32_t *const mine = tile + lane * kSnapPitch;
  for (uint32_t c0 = 0; c0 < L.rec_words; c0 += kSnapChunk) {
    const uint32_t c1 = min(c0 + kSnapChunk, L.rec_words);
    __syncthreads();
    const uint32_t nq = (c1 - c0) >> 2;
    for (uint32_t idx = threadIdx.x; idx < 64u * nq; idx += 256u) {
      const uint32_t rr = idx / nq, k = idx - rr * nq;
      const int32_t m = srec[rr];
      if (m >= 0) tile_write_quad(tile + rr * kSnapPitch, k, *(const uint4 *)(in + (size_t)m * L.rec_words + c0 + 4u * k));
    }
    __syncthreads();
    if (!act) continue;
    for (uint32_t k = 0; k < L.n_sec; k++) {
      const SnapSection sc = L.sec[k];
      const uint32_t lo = max(sc.w0, c0), hi = min(sc.w0 + sc.n * sc.e, c1);
      if (lo >= hi || sc.kind == SNAP_ZERO) continue;
      void *base = snap_base(D, sc.kind);
      for (uint32_t e = (lo - sc.w0) / sc.e + wv; e < (hi - sc.w0) / sc.e; e += 4u) {
        const uint32_t *t = mine + (sc.w0 + e * sc.e - c0);
        const size_t at = snap_elem(sc, e, i, n_dst, L.d);
        if (sc.e == 1) {
          uint32_t fresh = 0u;
          if (sc.kind == SNAP_IF) fresh = new_stream_int((int)e, N);
          else if (sc.kind == SNAP_RF) fresh = __builtin_bit_cast(uint32_t, (float)new_stream_real<Real>((int)e, N));
          ((uint32_t *)base)[at] = cont ? t[0] : fresh;
        } else if (sc.e == 2) {
          uint2 fresh = {0u, 0u};
          if (sc.kind == SNAP_RF) {
            const uint64_t b = __builtin_bit_cast(uint64_t, (double)new_stream_real<Real>((int)e, N));
            fresh.x = (uint32_t)b; fresh.y = (uint32_t)(b >> 32);
          }
          const uint2 v = {t[0], t[1]};
          ((uint2 *)base)[at] = cont ? v : fresh;
        } else {
          const uint4 z = {0u, 0u, 0u, 0u}, v = {t[0], t[1], t[2], t[3]};
          ((uint4 *)base)[at] = cont ? v : z;
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_snap_pack(const SnapLayout &L, const DemodState &S, uint32_t n_src, const int64_t *d_sel, uint32_t first, uint32_t count, void *d_out,
                            hipStream_t st) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(snap_pack_kernel, dim3((count + 63u) / 64u), dim3(256), 0, st, L, S, n_src, d_sel, first, count, (uint32_t *)d_out);
  return hipGetLastError();
}

hipError_t launch_snap_unpack(int precision, const SnapLayout &L, const DemodState &D, uint32_t n_dst, const int64_t *d_map, uint32_t rec_first, uint32_t rec_count,
                              bool fresh_too, const NewStream &N, const void *d_in, hipStream_t st) {
  if (n_dst == 0) return hipSuccess;
  const dim3 g((n_dst + 63u) / 64u), b(256);
  if (precision == 1) hipLaunchKernelGGL(snap_unpack_kernel<double>, g, b, 0, st, L, D, n_dst, d_map, rec_first, rec_count, fresh_too ? 1u : 0u, N, (const uint32_t *)d_in);
  else hipLaunchKernelGGL(snap_unpack_kernel<float>, g, b, 0, st, L, D, n_dst, d_map, rec_first, rec_count, fresh_too ? 1u : 0u, N, (const uint32_t *)d_in);
  return hipGetLastError();
}

}  // namespace fsk
