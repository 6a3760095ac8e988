// fsk_samples.hip -- the capture formats on both sides of the engine (include/fskhip.h: fskhip_sample_bytes, fskhip_ingest_device,
// fskhip_egress_device): 16-bit PCM, G.711 mu-law / A-law or float samples, stream-major [stream][sample] or as interleaved
// frames [sample][channel].
//   ingest   widens them into the float32 [stream][dst_pitch] rows every demodulator kernel reads.  The demodulators are SIMD-bound
//            at about a quarter of HBM, so the 4 B written and read again per sample go through bandwidth they leave idle.
//   egress   narrows the float32 [stream][src_pitch] rows the modulator writes.  d_lens (may be null): element (s, t) with
//            t >= d_lens[s] is the format's silence, whatever the source row holds there.
// The narrow samples are what crosses PCIe (fskhip_demodulate_host_fmt, fsk_dispatch.hip; fskhip_modulate_host_fmt, fsk_api.hip).
// Both directions are exact, and the tests compare bit for bit.  Formats, the stream-major row walk and the sample-major tile
// transpose are fsk_samples_dev.h's; the kernels here choose between them and say which index is the stream.  Neither writes
// outside elements (s < n_streams, t < n).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fsk_host.h"
#include "fsk_launch.h"
#include "fsk_samples_dev.h"

namespace fsk {

size_t sample_bytes(int format) {
  return format == FSKHIP_SAMPLES_F32 ? 4 : format == FSKHIP_SAMPLES_S16 ? 2 : (format == FSKHIP_SAMPLES_MULAW || format == FSKHIP_SAMPLES_ALAW) ? 1 : 0;
}

int check_sample_format(const char *who, int format, int layout) {
  if (!sample_bytes(format)) return fail(FSKHIP_E_INVALID, "%s: unknown sample format %d", who, format);
  if (layout != FSKHIP_LAYOUT_STREAM_MAJOR && layout != FSKHIP_LAYOUT_SAMPLE_MAJOR) return fail(FSKHIP_E_INVALID, "%s: unknown layout %d", who, layout);
  return FSKHIP_OK;
}

namespace {

static constexpr uint32_t kIngestQuads = 4;                                         // 16-byte vectors a lane keeps in flight (stream-major)
static constexpr uint32_t kIngestChunk = kSampleThreads * kIngestQuads * 4u;        // samples of a row per workgroup
static constexpr uint32_t kEgressFloats = 32;                                       // floats a lane keeps in flight (stream-major)
static constexpr uint32_t kEgressSpan = kSampleThreads * kEgressFloats;             // elements of a row per workgroup, in every format

// split: workgroups per row (stream-major) / 64-stream tiles per frame (sample-major), where neighbouring workgroups take
// neighbouring streams of the same frames; the grid is one-dimensional
template <int FMT, int LAYOUT>
__global__ __launch_bounds__(kSampleThreads) void ingest_kernel(const void *__restrict__ src_, size_t src_pitch, float *__restrict__ dst_, size_t dst_pitch,
                                                               uint32_t n_streams, size_t n, uint32_t split) {
  using F = SampleFmt<FMT>;
  const typename F::T *const src = (const typename F::T *)src_;
  uint32_t *const dst = (uint32_t *)dst_;
  const uint32_t hi = blockIdx.x / split, lo = blockIdx.x - hi * split;
  if constexpr (LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR) {
    using Quad = std::conditional_t<sizeof(typename F::T) == 4, uint4, std::conditional_t<sizeof(typename F::T) == 2, uint2, uint32_t>>;
    convert_row<kIngestQuads, Quad>(src + (size_t)hi * src_pitch, dst_ + (size_t)hi * dst_pitch, n, lo, [](typename F::T x, size_t) { return F::decode(x); });
  } else {   // rows = samples, columns = streams
    transpose_tile(src, src_pitch, n, n_streams, (size_t)hi * kSampleTile, lo * kSampleTile, nullptr, dst, dst_pitch,
                   [](uint32_t, size_t, typename F::T x) { return __float_as_uint(F::decode(x)); });
  }
}

template <int FMT, int LAYOUT>
__global__ __launch_bounds__(kSampleThreads) void egress_kernel(const float *__restrict__ src, size_t src_pitch, const uint32_t *__restrict__ d_lens,
                                                               void *__restrict__ dst_, size_t dst_pitch, uint32_t n_streams, size_t n, uint32_t split) {
  using F = SampleFmt<FMT>;
  typename F::Bits *const dst = (typename F::Bits *)dst_;
  const uint32_t hi = blockIdx.x / split, lo = blockIdx.x - hi * split;
  if constexpr (LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR) {
    size_t len = n;                                       // the row's elements that are conversions; silence from there on
    if (d_lens) len = d_lens[hi] < n ? (size_t)d_lens[hi] : n;
    convert_row<kEgressFloats * (uint32_t)sizeof(typename F::Bits) / 16u, float4>(src + (size_t)hi * src_pitch, dst + (size_t)hi * dst_pitch, n, lo,
                                                                         [len](float x, size_t t) { return t < len ? F::encode(x) : F::kSilence; });
  } else {   // rows = streams, columns = samples
    transpose_tile(src, src_pitch, n_streams, n, lo * kSampleTile, (size_t)hi * kSampleTile, d_lens, dst, dst_pitch,
                   [d_lens](uint32_t len, size_t t, float x) { return (!d_lens || t < len) ? F::encode(x) : F::kSilence; });
  }
}

// every instantiation of a kernel, once: [format][layout], in the order of include/fskhip.h's enums
#define FSK_SAMPLE_KERNELS(K)                                                                                        \
  {{FSK_K(K, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(K, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_SAMPLE_MAJOR)},     \
   {FSK_K(K, FSKHIP_SAMPLES_S16, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(K, FSKHIP_SAMPLES_S16, FSKHIP_LAYOUT_SAMPLE_MAJOR)},     \
   {FSK_K(K, FSKHIP_SAMPLES_MULAW, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(K, FSKHIP_SAMPLES_MULAW, FSKHIP_LAYOUT_SAMPLE_MAJOR)}, \
   {FSK_K(K, FSKHIP_SAMPLES_ALAW, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(K, FSKHIP_SAMPLES_ALAW, FSKHIP_LAYOUT_SAMPLE_MAJOR)}}
using IngestFn = void (*)(const void *, size_t, float *, size_t, uint32_t, size_t, uint32_t);
using EgressFn = void (*)(const float *, size_t, const uint32_t *, void *, size_t, uint32_t, size_t, uint32_t);
const KernelEntry<IngestFn> kIngestKernels[4][2] = FSK_SAMPLE_KERNELS(ingest_kernel);
const KernelEntry<EgressFn> kEgressKernels[4][2] = FSK_SAMPLE_KERNELS(egress_kernel);

// the one-dimensional grid of either kernel, `span` elements of a row per workgroup in stream-major layout: false where it is
// more workgroups than one launch takes
bool convert_grid(int layout, uint32_t n_streams, size_t n, uint32_t span, uint32_t *split, uint32_t *blocks) {
  uint64_t sp, bl;
  if (layout == FSKHIP_LAYOUT_STREAM_MAJOR) {
    sp = (n + span - 1u) / span;
    bl = sp * n_streams;
  } else {
    sp = (n_streams + kSampleTile - 1u) / kSampleTile;
    bl = sp * ((n + kSampleTile - 1u) / kSampleTile);
  }
  *split = (uint32_t)sp;
  *blocks = (uint32_t)bl;
  return bl <= 0x7FFFFFFFull;
}

// what is left of fskhip_ingest_device's / fskhip_egress_device's argument checks behind format, layout and the empty batch; the
// float side (ingest's destination, egress's source) is checked first
int check_convert_args(const char *who, bool float_is_dst, int layout, uint32_t n_streams, size_t n, const float *d_float, size_t float_pitch,
                       const void *d_narrow, size_t narrow_pitch, size_t esz, const uint32_t *d_lens) {
  if (!d_float || !d_narrow) return fail(FSKHIP_E_INVALID, "%s: null buffer", who);
  if (float_pitch < n) return fail(FSKHIP_E_INVALID, "%s: %s %zu < n_per_stream %zu", who, float_is_dst ? "dst_pitch" : "src_pitch", float_pitch, n);
  if (layout == FSKHIP_LAYOUT_STREAM_MAJOR && narrow_pitch < n)
    return fail(FSKHIP_E_INVALID, "%s: %s %zu < n_per_stream %zu", who, float_is_dst ? "src_pitch" : "dst_pitch", narrow_pitch, n);
  if (layout == FSKHIP_LAYOUT_SAMPLE_MAJOR && narrow_pitch < n_streams) return fail(FSKHIP_E_INVALID, "%s: frame pitch %zu < n_streams %u", who, narrow_pitch, n_streams);
  if ((reinterpret_cast<uintptr_t>(d_float) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_lens) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_narrow) & (esz - 1u)) != 0)
    return fail(FSKHIP_E_INVALID, "%s: a buffer is not aligned to its element size", who);
  return FSKHIP_OK;
}

int convert_result(const char *who, hipError_t err, uint32_t n_streams, size_t n) {
  if (err == hipErrorNoDevice) return fail(FSKHIP_E_NO_DEVICE, "no HIP device available (the engine has no CPU fallback)");
  if (err == hipErrorInvalidValue) return fail(FSKHIP_E_INVALID, "%s: %u streams x %zu samples are more workgroups than one launch takes", who, n_streams, n);
  HIP_TRY(err);
  return FSKHIP_OK;
}

}  // namespace

// (the caller has checked format, layout, pointers, alignments and pitches: the entry points below)
hipError_t launch_ingest(const void *d_src, int format, int layout, uint32_t n_streams, size_t n, size_t src_pitch, float *d_dst, size_t dst_pitch,
                         hipStream_t st) {
  if (n_streams == 0 || n == 0) return hipSuccess;
  uint32_t split, blocks;
  if (!convert_grid(layout, n_streams, n, kIngestChunk, &split, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kIngestKernels[format][layout].fn, dim3(blocks), dim3(kSampleThreads), 0, st, d_src, src_pitch, d_dst, dst_pitch, n_streams, n, split);
  return hipGetLastError();
}

hipError_t launch_egress(const float *d_src, size_t src_pitch, const uint32_t *d_lens, uint32_t n_streams, size_t n, int format, int layout, void *d_dst,
                         size_t dst_pitch, hipStream_t st) {
  if (n_streams == 0 || n == 0) return hipSuccess;
  uint32_t split, blocks;
  if (!convert_grid(layout, n_streams, n, kEgressSpan, &split, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kEgressKernels[format][layout].fn, dim3(blocks), dim3(kSampleThreads), 0, st, d_src, src_pitch, d_lens, d_dst, dst_pitch, n_streams, n, split);
  return hipGetLastError();
}

}  // namespace fsk

using namespace fsk;

extern "C" {
size_t fskhip_sample_bytes(int format) { return sample_bytes(format); }

int fskhip_ingest_device(const void *d_src, int format, int layout, uint32_t n_streams, size_t n, size_t src_pitch, float *d_dst, size_t dst_pitch,
                         void *hip_stream) {
  static const char who[] = "fskhip_ingest_device";
  if (const int rc = check_sample_format(who, format, layout)) return rc;
  if (n_streams == 0 || n == 0) return FSKHIP_OK;
  if (const int rc = check_convert_args(who, true, layout, n_streams, n, d_dst, dst_pitch, d_src, src_pitch, sample_bytes(format), nullptr)) return rc;
  return convert_result(who, launch_ingest(d_src, format, layout, n_streams, n, src_pitch, d_dst, dst_pitch, (hipStream_t)hip_stream), n_streams, n);
}

int fskhip_egress_device(const float *d_src, size_t src_pitch, const uint32_t *d_lens, uint32_t n_streams, size_t n, int format, int layout, void *d_dst,
                         size_t dst_pitch, void *hip_stream) {
  static const char who[] = "fskhip_egress_device";
  if (const int rc = check_sample_format(who, format, layout)) return rc;
  if (n_streams == 0 || n == 0) return FSKHIP_OK;
  if (const int rc = check_convert_args(who, false, layout, n_streams, n, d_src, src_pitch, d_dst, dst_pitch, sample_bytes(format), d_lens)) return rc;
  return convert_result(who, launch_egress(d_src, src_pitch, d_lens, n_streams, n, format, layout, d_dst, dst_pitch, (hipStream_t)hip_stream), n_streams, n);
}
}  // extern "C"
