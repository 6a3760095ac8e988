// fsk_egress.hip -- capture formats behind the modulator (include/fskhip.h: fskhip_egress_device, fskhip_modulate_host_fmt): the
// float32 [stream][src_pitch] rows the modulator writes, narrowed on the device into 16-bit PCM, G.711 mu-law / A-law or float
// samples, stream-major [stream][sample] or as interleaved frames [sample][channel].  The mirror of fsk_ingest.hip: the narrow
// samples are what crosses PCIe (fskhip_modulate_host_fmt, fsk_api.hip).
//
// The quantiser is include/fskhip.h's, formula for formula: round to nearest even, saturate, NaN = 0, then the standard G.711
// encoders with floor(log2) taken from the leading-zero count.  Every step is exact, and the tests compare bit for bit.
//
// d_lens (may be null): element (s, t) with t >= d_lens[s] is the format's silence, whatever the source row holds there.
//
//   stream-major   no LDS.  A row is a head of single elements up to the first 16-byte boundary of its DESTINATION, vectors of 16
//                  bytes -- 4 (f32), 8 (s16) or 16 (G.711) elements, one 16-byte store per vector, fed by float4 loads where the
//                  source lines up behind that head and by element loads where it does not --, and a tail of single elements.  A
//                  lane issues the loads of kEgressFloats floats before it converts the first; consecutive lanes stay on
//                  consecutive vectors on both sides.  A workgroup covers kEgressSpan elements of a row in every format.
//   sample-major   a transpose through LDS, one tile of 64 streams x 64 samples per workgroup (four waves).  Read side: lane =
//                  sample, a wave instruction is 64 consecutive floats (256 B) of one row; the lane converts, and the tile takes
//                  the CODE as a 32-bit word (d_lens[s] is one value per wave instruction there).  Write side: lane = stream, a
//                  wave instruction is 64 consecutive elements of one frame.  The tile is [stream][kEgressTilePitch] words with an
//                  odd pitch: the writes (word r * 65 + lane) and the reads (word lane * 65 + t) both put the 32 lanes of a half
//                  wave on 32 banks, as fsk_ingest.hip's tile does.  Partial tiles load nothing outside the source and store
//                  nothing outside [n][n_streams].
// Neither kernel writes outside elements (s < n_streams, t < n).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_host.h"
#include "fsk_launch.h"

namespace fsk {
namespace {

static constexpr uint32_t kEgressThreads = 256;
static constexpr uint32_t kEgressFloats = 32;                                   // floats a lane keeps in flight (stream-major)
static constexpr uint32_t kEgressSpan = kEgressThreads * kEgressFloats;         // elements of a row per workgroup
static constexpr uint32_t kEgressTile = 64;                                     // streams x samples per workgroup (sample-major)
static constexpr uint32_t kEgressTilePitch = kEgressTile + 1;                   // odd

// a format's element and its silence (what 0.0f encodes to)
template <int FMT> struct EgressElem;
template <> struct EgressElem<FSKHIP_SAMPLES_F32> { using T = uint32_t; static constexpr uint32_t kSilence = 0u; };
template <> struct EgressElem<FSKHIP_SAMPLES_S16> { using T = uint16_t; static constexpr uint32_t kSilence = 0u; };
template <> struct EgressElem<FSKHIP_SAMPLES_MULAW> { using T = uint8_t; static constexpr uint32_t kSilence = 0xFFu; };
template <> struct EgressElem<FSKHIP_SAMPLES_ALAW> { using T = uint8_t; static constexpr uint32_t kSilence = 0xD5u; };

// include/fskhip.h's encoders: the element's bits in the low end of a word (both G.711 encoders were held against Python's audioop
// for all 65 536 values, tests/test_egress_cpu.py)
template <int FMT>
__device__ __forceinline__ uint32_t egress_encode(float x) {
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

// E consecutive codes -> the 16 bytes they are in memory (little-endian)
template <uint32_t E>
__device__ __forceinline__ uint4 egress_pack(const uint32_t *c) {
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

// split: workgroups per row (stream-major) / 64-stream tiles per frame (sample-major); the grid is one-dimensional
template <int FMT, int LAYOUT>
__global__ __launch_bounds__(kEgressThreads) void egress_kernel(const float *__restrict__ src, size_t src_pitch, const uint32_t *__restrict__ d_lens,
                                                               void *__restrict__ dst_, size_t dst_pitch, uint32_t n_streams, size_t n, uint32_t split) {
  using T = typename EgressElem<FMT>::T;
  constexpr uint32_t kSilence = EgressElem<FMT>::kSilence;
  T *const dst = (T *)dst_;
  const uint32_t tid = threadIdx.x;
  if constexpr (LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR) {
    constexpr uint32_t E = 16u / sizeof(T);               // elements per 16-byte vector
    constexpr uint32_t K = kEgressFloats / E;             // vectors a lane keeps in flight
    const uint32_t s = blockIdx.x / split, c = blockIdx.x - s * split;
    const float *const in = src + (size_t)s * src_pitch;
    T *const out = dst + (size_t)s * dst_pitch;
    size_t len = n;                                       // the row's elements that are conversions; silence from there on
    if (d_lens) len = d_lens[s] < n ? (size_t)d_lens[s] : n;
    size_t head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / sizeof(T);   // elements up to the row's first 16-byte boundary
    head = head < n ? head : n;
    const size_t nv = (n - head) / E, tail0 = head + (size_t)E * nv;
    if (c == 0) {   // the row's single elements: at most E - 1 in front, E - 1 behind
      if (tid < head) out[tid] = (T)(tid < len ? egress_encode<FMT>(in[tid]) : kSilence);
      const size_t t = tail0 + (tid - 64u);
      if (tid >= 64u && t < n) out[t] = (T)(t < len ? egress_encode<FMT>(in[t]) : kSilence);
    }
    const float *const vin = in + head;
    T *const vout = out + head;
    const size_t q0 = (size_t)c * (kEgressThreads * K) + tid;
    float f[K][E];
    if ((reinterpret_cast<uintptr_t>(vin) & 15u) == 0) {   // (uniform over the workgroup: a property of the row)
#pragma unroll
      for (uint32_t k = 0; k < K; k++) {
        const size_t q = q0 + (size_t)k * kEgressThreads;
        if (q < nv) {
#pragma unroll
          for (uint32_t j = 0; j < E / 4u; j++) {
            const float4 w = *(const float4 *)(vin + (size_t)E * q + 4u * j);
            f[k][4 * j] = w.x; f[k][4 * j + 1] = w.y; f[k][4 * j + 2] = w.z; f[k][4 * j + 3] = w.w;
          }
        }
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < K; k++) {
        const size_t q = q0 + (size_t)k * kEgressThreads;
        if (q < nv) {
#pragma unroll
          for (uint32_t i = 0; i < E; i++) f[k][i] = vin[(size_t)E * q + i];
        }
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
      const size_t q = q0 + (size_t)k * kEgressThreads;
      if (q < nv) {
        const size_t t = head + (size_t)E * q;
        uint32_t code[E];
#pragma unroll
        for (uint32_t i = 0; i < E; i++) code[i] = t + i < len ? egress_encode<FMT>(f[k][i]) : kSilence;
        *(uint4 *)(vout + (size_t)E * q) = egress_pack<E>(code);
      }
    }
  } else {
    __shared__ uint32_t tile[kEgressTile * kEgressTilePitch];
    const uint32_t tt = blockIdx.x / split, ts = blockIdx.x - tt * split;   // neighbouring workgroups: neighbouring streams of the same frames
    const uint32_t s0 = ts * kEgressTile, lane = tid & 63u, wv = tid >> 6;
    const size_t t0 = (size_t)tt * kEgressTile;
    constexpr uint32_t kRows = kEgressTile / (kEgressThreads / 64u);   // rows of the tile per wave, on either side
    const size_t t = t0 + lane;
    float v[kRows];
    uint32_t len[kRows];
#pragma unroll
    for (uint32_t j = 0; j < kRows; j++) {
      const uint32_t s = s0 + wv + 4u * j;
      const bool ok = s < n_streams && t < n;
      v[j] = ok ? src[(size_t)s * src_pitch + t] : 0.0f;
      len[j] = (d_lens && s < n_streams) ? d_lens[s] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < kRows; j++) tile[(wv + 4u * j) * kEgressTilePitch + lane] = (!d_lens || t < len[j]) ? egress_encode<FMT>(v[j]) : kSilence;
    __syncthreads();
    const bool s_ok = s0 + lane < n_streams;
#pragma unroll
    for (uint32_t j = 0; j < kRows; j++) {
      const uint32_t r = wv + 4u * j;
      if (s_ok && t0 + r < n) dst[(t0 + r) * dst_pitch + s0 + lane] = (T)tile[lane * kEgressTilePitch + r];
    }
  }
}

using EgressFn = void (*)(const float *, size_t, const uint32_t *, void *, size_t, uint32_t, size_t, uint32_t);
// every instantiation, once: [format][layout], in the order of include/fskhip.h's enums
const KernelEntry<EgressFn> kEgressKernels[4][2] = {
    {FSK_K(egress_kernel, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(egress_kernel, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_SAMPLE_MAJOR)},
    {FSK_K(egress_kernel, FSKHIP_SAMPLES_S16, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(egress_kernel, FSKHIP_SAMPLES_S16, FSKHIP_LAYOUT_SAMPLE_MAJOR)},
    {FSK_K(egress_kernel, FSKHIP_SAMPLES_MULAW, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(egress_kernel, FSKHIP_SAMPLES_MULAW, FSKHIP_LAYOUT_SAMPLE_MAJOR)},
    {FSK_K(egress_kernel, FSKHIP_SAMPLES_ALAW, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(egress_kernel, FSKHIP_SAMPLES_ALAW, FSKHIP_LAYOUT_SAMPLE_MAJOR)},
};

}  // namespace

// (the caller has checked format, layout, pointers, alignments and pitches: fskhip_egress_device below)
hipError_t launch_egress(const float *d_src, size_t src_pitch, const uint32_t *d_lens, uint32_t n_streams, size_t n, int format, int layout, void *d_dst,
                         size_t dst_pitch, hipStream_t st) {
  if (n_streams == 0 || n == 0) return hipSuccess;
  uint64_t split, blocks;
  if (layout == FSKHIP_LAYOUT_STREAM_MAJOR) {
    split = (n + kEgressSpan - 1u) / kEgressSpan;
    blocks = split * n_streams;
  } else {
    split = (n_streams + kEgressTile - 1u) / kEgressTile;
    blocks = split * ((n + kEgressTile - 1u) / kEgressTile);
  }
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kEgressKernels[format][layout].fn, dim3((uint32_t)blocks), dim3(kEgressThreads), 0, st, d_src, src_pitch, d_lens, d_dst, dst_pitch, n_streams,
                     n, (uint32_t)split);
  return hipGetLastError();
}

}  // namespace fsk

using namespace fsk;

extern "C" {
int fskhip_egress_device(const float *d_src, size_t src_pitch, const uint32_t *d_lens, uint32_t n_streams, size_t n, int format, int layout, void *d_dst,
                         size_t dst_pitch, void *hip_stream) {
  const size_t esz = ingest_sample_bytes(format);
  if (!esz) return fail(FSKHIP_E_INVALID, "fskhip_egress_device: unknown sample format %d", format);
  if (layout != FSKHIP_LAYOUT_STREAM_MAJOR && layout != FSKHIP_LAYOUT_SAMPLE_MAJOR) return fail(FSKHIP_E_INVALID, "fskhip_egress_device: unknown layout %d", layout);
  if (n_streams == 0 || n == 0) return FSKHIP_OK;
  if (!d_src || !d_dst) return fail(FSKHIP_E_INVALID, "fskhip_egress_device: null buffer");
  if (src_pitch < n) return fail(FSKHIP_E_INVALID, "fskhip_egress_device: src_pitch %zu < n_per_stream %zu", src_pitch, n);
  if (layout == FSKHIP_LAYOUT_STREAM_MAJOR && dst_pitch < n) return fail(FSKHIP_E_INVALID, "fskhip_egress_device: dst_pitch %zu < n_per_stream %zu", dst_pitch, n);
  if (layout == FSKHIP_LAYOUT_SAMPLE_MAJOR && dst_pitch < n_streams)
    return fail(FSKHIP_E_INVALID, "fskhip_egress_device: frame pitch %zu < n_streams %u", dst_pitch, n_streams);
  if ((reinterpret_cast<uintptr_t>(d_src) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_lens) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_dst) & (esz - 1u)) != 0)
    return fail(FSKHIP_E_INVALID, "fskhip_egress_device: a buffer is not aligned to its element size");
  const hipError_t err = launch_egress(d_src, src_pitch, d_lens, n_streams, n, format, layout, d_dst, dst_pitch, (hipStream_t)hip_stream);
  if (err == hipErrorNoDevice) return fail(FSKHIP_E_NO_DEVICE, "no HIP device available (the engine has no CPU fallback)");
  if (err == hipErrorInvalidValue) return fail(FSKHIP_E_INVALID, "fskhip_egress_device: %u streams x %zu samples are more workgroups than one launch takes", n_streams, n);
  HIP_TRY(err);
  return FSKHIP_OK;
}
}  // extern "C"
