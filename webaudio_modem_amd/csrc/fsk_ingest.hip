// fsk_ingest.hip -- capture formats in front of the demodulators (include/fskhip.h: fskhip_ingest_device, fskhip_sample_bytes):
// 16-bit PCM, G.711 mu-law / A-law or float samples, stream-major [stream][sample] or as interleaved capture frames
// [sample][channel], widened on the device into the float32 [stream][dst_pitch] rows every demodulator kernel reads.  The narrow
// samples are what crosses PCIe (fskhip_demodulate_host_fmt, fsk_dispatch.hip); the demodulators are SIMD-bound at about a
// quarter of HBM, so the 4 B written and read again per sample here go through bandwidth they leave idle.
//
// Every value is an integer of at most 16 bits times 2^-15: the float is exact, and the tests compare bit for bit.
//
//   stream-major   no LDS.  A row is a head of single elements up to the first 16-byte boundary of its DESTINATION (the host
//                  path hands over rows that start three floats into an aligned one, host_stage_shift, fsk_plan.h), quads of
//                  four elements -- one float4 store per quad, fed by one 16- / 8- / 4-byte load where the source lines up
//                  with its own quad size behind that head and by four element loads where it does not --, and a tail of
//                  single elements.  A lane issues the loads of kIngestQuads quads before it converts the first, and
//                  consecutive lanes stay on consecutive addresses on both sides.
//   sample-major   a transpose through LDS, one tile of 64 streams x 64 samples per workgroup (four waves).  Read side: lane =
//                  stream, a wave instruction is 64 consecutive elements of one frame.  Write side: lane = sample, 64
//                  consecutive floats (256 B) of one row; dword stores, so every destination alignment is the same path.
//                  The tile is [stream][kIngestTilePitch] words with an odd pitch: the writes (word lane * 65 + t) and the reads
//                  (word r * 65 + lane) both put the 32 lanes of a half wave on 32 banks (ds_write_b32 / ds_read_b32: bank =
//                  word mod 32 within a half), as fsk_snapshot.hip's 129-word pitch does.  Partial tiles in both directions
//                  load zeros and store nothing.
// Neither kernel writes outside [0, n) of a row.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_host.h"
#include "fsk_launch.h"

namespace fsk {

size_t ingest_sample_bytes(int format) {
  return format == FSKHIP_SAMPLES_F32 ? 4 : format == FSKHIP_SAMPLES_S16 ? 2 : (format == FSKHIP_SAMPLES_MULAW || format == FSKHIP_SAMPLES_ALAW) ? 1 : 0;
}

namespace {

static constexpr uint32_t kIngestThreads = 256;
static constexpr uint32_t kIngestQuads = 4;                                      // quads a lane keeps in flight (stream-major)
static constexpr uint32_t kIngestChunk = kIngestThreads * kIngestQuads * 4u;     // samples of a row per workgroup
static constexpr uint32_t kIngestTile = 64;                                      // streams x samples per workgroup (sample-major)
static constexpr uint32_t kIngestTilePitch = kIngestTile + 1;                    // odd

// a format's element, and the one load that brings four of them
template <int FMT> struct IngestElem;
template <> struct IngestElem<FSKHIP_SAMPLES_F32> { using T = float; using Q = float4; };
template <> struct IngestElem<FSKHIP_SAMPLES_S16> { using T = int16_t; using Q = uint2; };
template <> struct IngestElem<FSKHIP_SAMPLES_MULAW> { using T = uint8_t; using Q = uint32_t; };
template <> struct IngestElem<FSKHIP_SAMPLES_ALAW> { using T = uint8_t; using Q = uint32_t; };

// include/fskhip.h's table, formula for formula (G.711 as in ITU-T's reference expansion; both were held against Python's audioop
// for all 256 codes, tests/test_ingest_cpu.py)
template <int FMT>
__device__ __forceinline__ float ingest_decode(typename IngestElem<FMT>::T x) {
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

// split: workgroups per row (stream-major) / 64-stream tiles per frame (sample-major); the grid is one-dimensional
template <int FMT, int LAYOUT>
__global__ __launch_bounds__(kIngestThreads) void ingest_kernel(const void *__restrict__ src_, size_t src_pitch, float *__restrict__ dst, size_t dst_pitch,
                                                               uint32_t n_streams, size_t n, uint32_t split) {
  using T = typename IngestElem<FMT>::T;
  using Q = typename IngestElem<FMT>::Q;
  const T *const src = (const T *)src_;
  const uint32_t tid = threadIdx.x;
  if constexpr (LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR) {
    const uint32_t s = blockIdx.x / split, c = blockIdx.x - s * split;
    const T *const in = src + (size_t)s * src_pitch;
    float *const out = dst + (size_t)s * dst_pitch;
    size_t head = (4u - (uint32_t)((reinterpret_cast<uintptr_t>(out) >> 2) & 3u)) & 3u;   // elements up to the row's first 16-byte boundary
    head = head < n ? head : n;
    const size_t nq = (n - head) >> 2, tail0 = head + 4u * nq;
    if (c == 0) {   // the row's single elements: at most three in front, three behind
      if (tid < head) out[tid] = ingest_decode<FMT>(in[tid]);
      if (tid >= 64u && tail0 + (tid - 64u) < n) out[tail0 + (tid - 64u)] = ingest_decode<FMT>(in[tail0 + (tid - 64u)]);
    }
    const T *const qin = in + head;
    float *const qout = out + head;
    const size_t q0 = (size_t)c * (kIngestThreads * kIngestQuads) + tid;
    T v[kIngestQuads][4];
    if ((reinterpret_cast<uintptr_t>(qin) & (sizeof(Q) - 1u)) == 0) {   // (uniform over the workgroup: a property of the row)
#pragma unroll
      for (uint32_t k = 0; k < kIngestQuads; k++) {
        const size_t q = q0 + (size_t)k * kIngestThreads;
        if (q < nq) {
          const Q w = *(const Q *)(qin + 4u * q);
          __builtin_memcpy(v[k], &w, sizeof(Q));
        }
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < kIngestQuads; k++) {
        const size_t q = q0 + (size_t)k * kIngestThreads;
        if (q < nq) {
#pragma unroll
          for (uint32_t i = 0; i < 4; i++) v[k][i] = qin[4u * q + i];
        }
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < kIngestQuads; k++) {
      const size_t q = q0 + (size_t)k * kIngestThreads;
      if (q < nq) {
        float4 f;
        f.x = ingest_decode<FMT>(v[k][0]); f.y = ingest_decode<FMT>(v[k][1]);
        f.z = ingest_decode<FMT>(v[k][2]); f.w = ingest_decode<FMT>(v[k][3]);
        *(float4 *)(qout + 4u * q) = f;
      }
    }
  } else {
    __shared__ float tile[kIngestTile * kIngestTilePitch];
    const uint32_t tt = blockIdx.x / split, ts = blockIdx.x - tt * split;   // neighbouring workgroups: neighbouring streams of the same frames
    const uint32_t s0 = ts * kIngestTile, lane = tid & 63u, wv = tid >> 6;
    const size_t t0 = (size_t)tt * kIngestTile;
    constexpr uint32_t kRows = kIngestTile / (kIngestThreads / 64u);   // rows of the tile per wave, on either side
    const bool s_ok = s0 + lane < n_streams;
    T v[kRows];
#pragma unroll
    for (uint32_t j = 0; j < kRows; j++) {
      const size_t t = t0 + wv + 4u * j;
      v[j] = (s_ok && t < n) ? src[t * src_pitch + s0 + lane] : T(0);
    }
#pragma unroll
    for (uint32_t j = 0; j < kRows; j++) tile[lane * kIngestTilePitch + wv + 4u * j] = ingest_decode<FMT>(v[j]);
    __syncthreads();
    const bool t_ok = t0 + lane < n;
#pragma unroll
    for (uint32_t j = 0; j < kRows; j++) {
      const uint32_t r = wv + 4u * j;
      if (t_ok && s0 + r < n_streams) dst[(size_t)(s0 + r) * dst_pitch + t0 + lane] = tile[r * kIngestTilePitch + lane];
    }
  }
}

using IngestFn = void (*)(const void *, size_t, float *, size_t, uint32_t, size_t, uint32_t);
// every instantiation, once: [format][layout], in the order of include/fskhip.h's enums
const KernelEntry<IngestFn> kIngestKernels[4][2] = {
    {FSK_K(ingest_kernel, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(ingest_kernel, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_SAMPLE_MAJOR)},
    {FSK_K(ingest_kernel, FSKHIP_SAMPLES_S16, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(ingest_kernel, FSKHIP_SAMPLES_S16, FSKHIP_LAYOUT_SAMPLE_MAJOR)},
    {FSK_K(ingest_kernel, FSKHIP_SAMPLES_MULAW, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(ingest_kernel, FSKHIP_SAMPLES_MULAW, FSKHIP_LAYOUT_SAMPLE_MAJOR)},
    {FSK_K(ingest_kernel, FSKHIP_SAMPLES_ALAW, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(ingest_kernel, FSKHIP_SAMPLES_ALAW, FSKHIP_LAYOUT_SAMPLE_MAJOR)},
};

}  // namespace

// (the caller has checked format, layout, pointers, alignments and pitches: fskhip_ingest_device below)
hipError_t launch_ingest(const void *d_src, int format, int layout, uint32_t n_streams, size_t n, size_t src_pitch, float *d_dst, size_t dst_pitch,
                         hipStream_t st) {
  if (n_streams == 0 || n == 0) return hipSuccess;
  uint64_t split, blocks;
  if (layout == FSKHIP_LAYOUT_STREAM_MAJOR) {
    split = (n + kIngestChunk - 1u) / kIngestChunk;
    blocks = split * n_streams;
  } else {
    split = (n_streams + kIngestTile - 1u) / kIngestTile;
    blocks = split * ((n + kIngestTile - 1u) / kIngestTile);
  }
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kIngestKernels[format][layout].fn, dim3((uint32_t)blocks), dim3(kIngestThreads), 0, st, d_src, src_pitch, d_dst, dst_pitch, n_streams, n,
                     (uint32_t)split);
  return hipGetLastError();
}

}  // namespace fsk

using namespace fsk;

extern "C" {
size_t fskhip_sample_bytes(int format) { return ingest_sample_bytes(format); }

int fskhip_ingest_device(const void *d_src, int format, int layout, uint32_t n_streams, size_t n, size_t src_pitch, float *d_dst, size_t dst_pitch,
                         void *hip_stream) {
  const size_t esz = ingest_sample_bytes(format);
  if (!esz) return fail(FSKHIP_E_INVALID, "fskhip_ingest_device: unknown sample format %d", format);
  if (layout != FSKHIP_LAYOUT_STREAM_MAJOR && layout != FSKHIP_LAYOUT_SAMPLE_MAJOR) return fail(FSKHIP_E_INVALID, "fskhip_ingest_device: unknown layout %d", layout);
  if (n_streams == 0 || n == 0) return FSKHIP_OK;
  if (!d_src || !d_dst) return fail(FSKHIP_E_INVALID, "fskhip_ingest_device: null buffer");
  if (dst_pitch < n) return fail(FSKHIP_E_INVALID, "fskhip_ingest_device: dst_pitch %zu < n_per_stream %zu", dst_pitch, n);
  if (layout == FSKHIP_LAYOUT_STREAM_MAJOR && src_pitch < n) return fail(FSKHIP_E_INVALID, "fskhip_ingest_device: src_pitch %zu < n_per_stream %zu", src_pitch, n);
  if (layout == FSKHIP_LAYOUT_SAMPLE_MAJOR && src_pitch < n_streams)
    return fail(FSKHIP_E_INVALID, "fskhip_ingest_device: frame pitch %zu < n_streams %u", src_pitch, n_streams);
  if ((reinterpret_cast<uintptr_t>(d_src) & (esz - 1u)) != 0 || (reinterpret_cast<uintptr_t>(d_dst) & 3u) != 0)
    return fail(FSKHIP_E_INVALID, "fskhip_ingest_device: a buffer is not aligned to its element size");
  const hipError_t err = launch_ingest(d_src, format, layout, n_streams, n, src_pitch, d_dst, dst_pitch, (hipStream_t)hip_stream);
  if (err == hipErrorNoDevice) return fail(FSKHIP_E_NO_DEVICE, "no HIP device available (the engine has no CPU fallback)");
  if (err == hipErrorInvalidValue) return fail(FSKHIP_E_INVALID, "fskhip_ingest_device: %u streams x %zu samples are more workgroups than one launch takes", n_streams, n);
  HIP_TRY(err);
  return FSKHIP_OK;
}
}  // extern "C"
