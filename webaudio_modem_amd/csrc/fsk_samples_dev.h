// fsk_samples_dev.h -- the capture formats on the device (include/fskhip.h: FSKHIP_SAMPLES_*), once for both directions of
// fsk_samples.hip: a format's element, silence and conversions (SampleFmt), the walk along a stream-major row (convert_row) and
// the transpose of a 64 x 64 tile through LDS (transpose_tile).  Elements travel as their bits in the low end of a 32-bit word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/fskhip.h"

namespace fsk {

static constexpr uint32_t kSampleThreads = 256;   // four waves per workgroup in both layouts
static constexpr uint32_t kSampleTile = 64;       // rows x columns of a transposed tile

// A format: its element (T as a value, Bits as it is stored), its silence (what 0.0f encodes to) and include/fskhip.h's table and
// encoders, formula for formula.  decode is exact: an integer of at most 16 bits times 2^-15.  encode rounds to nearest even,
// saturates, takes NaN as 0, then the standard G.711 encoders with floor(log2) from the leading-zero count; every step is exact.
// (Both directions were held against Python's audioop: all 256 codes, tests/test_ingest_cpu.py; all 65 536 values,
// tests/test_egress_cpu.py.)
template <int FMT>
struct SampleFmt {
  using T = std::conditional_t<FMT == FSKHIP_SAMPLES_F32, float, std::conditional_t<FMT == FSKHIP_SAMPLES_S16, int16_t, uint8_t>>;
  using Bits = std::conditional_t<FMT == FSKHIP_SAMPLES_F32, uint32_t, std::conditional_t<FMT == FSKHIP_SAMPLES_S16, uint16_t, uint8_t>>;
  static constexpr uint32_t kSilence = FMT == FSKHIP_SAMPLES_MULAW ? 0xFFu : FMT == FSKHIP_SAMPLES_ALAW ? 0xD5u : 0u;

  static __device__ __forceinline__ float decode(T x) {
    if constexpr (FMT == FSKHIP_SAMPLES_F32) {
      return x;
    } else if constexpr (FMT == FSKHIP_SAMPLES_S16) {
      return (float)x * (1.0f / 32768.0f);
    } else if constexpr (FMT == FSKHIP_SAMPLES_MULAW) {
      const uint32_t u = ~(uint32_t)x & 0xFFu;
      const int32_t mag = (int32_t)((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u)) - 0x84;
      return (float)((u & 0x80u) ? -mag : mag) * (1.0f / 32768.0f);
    } else {
      const uint32_t a = (uint32_t)x ^ 0x55u;
      const uint32_t e = (a >> 4) & 7u, m = a & 15u;
      const int32_t mag = (int32_t)(e ? ((m << 4) + 0x108u) << (e - 1u) : (m << 4) + 8u);
      return (float)((a & 0x80u) ? mag : -mag) * (1.0f / 32768.0f);
    }
  }

  static __device__ __forceinline__ uint32_t encode(float x) {
    if constexpr (FMT == FSKHIP_SAMPLES_F32) {
      return __float_as_uint(x);
    } else {
      float y = __builtin_rintf(x * 32768.0f);   // (exact product; round to nearest even)
      y = (y != y) ? 0.0f : y;
      y = __builtin_fminf(__builtin_fmaxf(y, -32768.0f), 32767.0f);
      const int32_t v = (int32_t)y;
      if constexpr (FMT == FSKHIP_SAMPLES_S16) {
        return (uint32_t)v & 0xFFFFu;
      } else if constexpr (FMT == FSKHIP_SAMPLES_MULAW) {
        int32_t m = v >> 2;
        const bool neg = m < 0;
        m = neg ? -m : m;
        m = (m < 8158 ? m : 8158) + 33;                          // 33 .. 8191
        const uint32_t seg = 26u - (uint32_t)__builtin_clz((uint32_t)m);   // floor(log2 m) - 5: 0 .. 7
        return ((seg << 4) | (((uint32_t)m >> (seg + 1u)) & 15u)) ^ (neg ? 0x7Fu : 0xFFu);
      } else {
        int32_t m = v >> 3;
        const bool neg = m < 0;
        m = neg ? -m - 1 : m;                                    // 0 .. 4095
        const uint32_t lg = 31u - (uint32_t)__builtin_clz((uint32_t)(m | 1));
        const uint32_t seg = lg > 4u ? lg - 4u : 0u;             // 0 .. 7
        return ((seg << 4) | (((uint32_t)m >> (seg < 2u ? 1u : seg)) & 15u)) ^ (neg ? 0x55u : 0xD5u);
      }
    }
  }
};

// E consecutive elements' words -> the 16 bytes they are in memory (little-endian)
template <uint32_t E>
__device__ __forceinline__ uint4 pack16(const uint32_t *c) {
  uint32_t w[4];
  if constexpr (E == 4) {
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) w[i] = c[i];
  } else if constexpr (E == 8) {
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) w[i] = c[2 * i] | (c[2 * i + 1] << 16);
  } else {
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) w[i] = c[4 * i] | (c[4 * i + 1] << 8) | (c[4 * i + 2] << 16) | (c[4 * i + 3] << 24);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// Four consecutive source elements in one load of type Wide, p aligned to it: through the members of HIP's vector of four Src, or
// through any other type of the four's size (an integer, uint2, uint4) and a copy of its bytes.  Either is one load instruction; the
// compiler shares such loads between convert_row's two paths differently, and each kernel names the form that leaves it the parent
// commit's count of memory instructions (profiles/samples_refactor_static.txt).
template <typename Wide, typename Src>
__device__ __forceinline__ void load4(const Src *p, Src *v) {
  static_assert(sizeof(Wide) == 4 * sizeof(Src) && sizeof(Wide) <= 16, "one load of four elements, at most 16 bytes");
  const Wide w = *(const Wide *)p;
  if constexpr (std::is_same<Wide, HIP_vector_type<Src, 4>>::value) {
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
  } else {
    __builtin_memcpy(v, &w, sizeof(Wide));
  }
}

// One stream-major row, n elements of Src at `in` -> Dst at `out`, by workgroup c of the row's; conv(source value, sample index t)
// gives element t: a Dst where that has four bytes (float, or a float's bits), else an unsigned Dst's bits in a word.  No LDS.  The row is a head of single elements up to the first
// 16-byte boundary of its DESTINATION (the demodulate host path hands over rows that start three floats into an aligned one,
// host_stage_shift, fsk_plan.h), vectors of E = 16 / sizeof(Dst) elements -- one 16-byte store per vector, fed by loads of four
// elements (Wide, load4) where the source lines up with them behind that head and by E element loads where it does not --, and a tail of single
// elements; head and tail are workgroup 0's.  A lane issues the loads of K vectors before it converts the first, consecutive
// lanes stay on consecutive vectors on both sides, and a workgroup covers kSampleThreads * K * E elements.  Nothing is written
// outside [0, n).
template <uint32_t K, typename Wide, typename Src, typename Dst, typename Conv>
__device__ __forceinline__ void convert_row(const Src *__restrict__ in, Dst *__restrict__ out, size_t n, uint32_t c, Conv conv) {
  constexpr uint32_t E = 16u / sizeof(Dst);
  static_assert(E % 4u == 0, "a vector is fed by whole loads of four elements (load4)");
  const uint32_t tid = threadIdx.x;
  size_t head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / sizeof(Dst);
  head = head < n ? head : n;
  const size_t nv = (n - head) / E, tail0 = head + (size_t)E * nv;
  if (c == 0) {   // the row's single elements: at most E - 1 in front, E - 1 behind
    if (tid < head) out[tid] = (Dst)conv(in[tid], (size_t)tid);
    const size_t t = tail0 + (tid - 64u);
    if (tid >= 64u && t < n) out[t] = (Dst)conv(in[t], t);
  }
  const Src *const vin = in + head;
  Dst *const vout = out + head;
  const size_t q0 = (size_t)c * (kSampleThreads * K) + tid;
  Src v[K][E];
  if ((reinterpret_cast<uintptr_t>(vin) & (sizeof(Wide) - 1u)) == 0) {   // (uniform over the workgroup: a property of the row)
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
      const size_t q = q0 + (size_t)k * kSampleThreads;
      if (q < nv) {
#pragma unroll
        for (uint32_t j = 0; j < E / 4u; j++) load4<Wide>(vin + (size_t)E * q + 4u * j, &v[k][4u * j]);
      }
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
      const size_t q = q0 + (size_t)k * kSampleThreads;
      if (q < nv) {
#pragma unroll
        for (uint32_t i = 0; i < E; i++) v[k][i] = vin[(size_t)E * q + i];
      }
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    const size_t q = q0 + (size_t)k * kSampleThreads;
    if (q < nv) {
      const size_t t = head + (size_t)E * q;
      decltype(conv(v[k][0], t)) w[E];
#pragma unroll
      for (uint32_t i = 0; i < E; i++) w[i] = conv(v[k][i], t + i);
      if constexpr (E == 4) {
        HIP_vector_type<Dst, 4> o;
        o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
        *(HIP_vector_type<Dst, 4> *)(vout + (size_t)E * q) = o;
      } else {
        *(uint4 *)(vout + (size_t)E * q) = pack16<E>(w);
      }
    }
  }
}

// One 64 x 64 tile of a transpose, src[row][col] -> dst[col][row] (Dst an unsigned integer: the bits), rows from row0 and columns
// from col0, by one workgroup of four waves; each wave takes 16 rows of the tile on either side.  Read side: lane = column, a wave
// instruction is 64 consecutive elements of one source row; the lane converts, and the tile takes conv(row word, col, value) as a
// 32-bit word.  row_words (may be null): one word per source row, fetched with that row's loads -- one value per wave instruction
// -- and handed to conv (0 where null).  Write side: lane = row, a wave instruction is 64 consecutive elements of one
// destination row; single-element stores, so every destination alignment is the same path.  The tile is [row][65] words: the odd
// pitch puts the writes (word r * 65 + lane) and the reads (word lane * 65 + c) of the 32 lanes of a half wave on 32 banks
// (ds_write_b32 / ds_read_b32: bank = word mod 32 within a half), as fsk_snapshot.hip's 129-word pitch does.  Partial tiles load
// zeros outside the source and store nothing outside [n_cols][n_rows].  Row and Col are the index types: 32 bits for streams, size_t
// for samples.
template <typename Src, typename Dst, typename Row, typename Col, typename Conv>
__device__ __forceinline__ void transpose_tile(const Src *__restrict__ src, size_t src_pitch, Row n_rows, Col n_cols, Row row0, Col col0,
                                               const uint32_t *__restrict__ row_words, Dst *__restrict__ dst, size_t dst_pitch, Conv conv) {
  constexpr uint32_t kPitch = kSampleTile + 1;                       // odd
  constexpr uint32_t kWaves = kSampleThreads / 64u;
  constexpr uint32_t kRows = kSampleTile / kWaves;                   // rows of the tile per wave, on either side
  __shared__ uint32_t tile[kSampleTile * kPitch];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const Col col = col0 + lane;
  Src v[kRows];
  uint32_t rw[kRows];
#pragma unroll
  for (uint32_t j = 0; j < kRows; j++) {
    const Row row = row0 + wv + kWaves * j;
    v[j] = (row < n_rows && col < n_cols) ? src[(size_t)row * src_pitch + col] : Src(0);
    rw[j] = (row_words && row < n_rows) ? row_words[row] : 0u;
  }
#pragma unroll
  for (uint32_t j = 0; j < kRows; j++) tile[(wv + kWaves * j) * kPitch + lane] = conv(rw[j], col, v[j]);
  __syncthreads();
  const bool row_ok = row0 + lane < n_rows;
#pragma unroll
  for (uint32_t j = 0; j < kRows; j++) {
    const uint32_t c = wv + kWaves * j;
    if (row_ok && col0 + c < n_cols) dst[(size_t)(col0 + c) * dst_pitch + row0 + lane] = (Dst)tile[lane * kPitch + c];
  }
}

}  // namespace fsk
