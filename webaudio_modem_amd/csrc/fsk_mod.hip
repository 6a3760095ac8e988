// fsk_mod.hip -- FSK modulator (FSKCore.modulateData, src/modems/fsk.ts:377-424), the synthetic
// multi-frame workload generator and the AWGN kernels, for gfx950.
//
// One lane per stream, like the demodulator: the reference's phase is an UNWRAPPED f64 that is
// advanced by `phase += 2*pi*f/sr` once per sample and carried across bits (fsk.ts:398-406), so
// reproducing its roundings means performing the same chain of f64 additions in order; the
// samples of a stream are therefore produced sequentially by one lane, 32 at a time into an
// LDS tile that the wave then stores as coalesced 16-B/lane row segments (the mirror image of
// the demodulator's tile load).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fsk_fdlibm.h"
#include "fsk_params.h"
#include "fsk_wait.h"
#include "fsk_launch.h"
#include "fsk_samples_dev.h"
#include "fsk_mac_dev.h"
#include "fsk_processor_rate_plan.h"

namespace fsk {

__host__ __device__ inline uint64_t fmix64(uint64_t z) {  // splitmix64 finaliser
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
static constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ inline uint8_t synth_payload_byte(uint64_t seed, uint32_t stream, uint32_t frame, uint32_t i) {
  uint64_t x = fmix64(seed + kGolden * (1ull + stream));
  x = fmix64(x ^ (kGolden * (1ull + frame)));
  x = fmix64(x + kGolden * (1ull + i));
  return (uint8_t)(x >> 56);
}
__host__ __device__ inline void synth_stream_params(uint64_t seed, uint32_t stream, uint32_t lead_max,
                                                    double amp_lo, double amp_hi, uint32_t *lead, double *amp) {
  uint64_t a = fmix64((seed ^ 0xA5A5A5A5A5A5A5A5ull) + kGolden * (1ull + stream));
  uint64_t b = fmix64(a + kGolden);
  *lead = (uint32_t)(a % ((uint64_t)lead_max + 1ull));
  double u = (double)(b >> 11) * (1.0 / 9007199254740992.0);
  *amp = amp_lo + (amp_hi - amp_lo) * u;
}

// Sequential generator of one frame = what generateFSKSignalInternal() writes (fsk.ts:389-424):
// 2*spb zeros, then for preamble|sfd|data bytes: start bits (0), 8 data bits MSB first, optional
// parity, stop bits (1), each bit spb samples of sin(phase) with phase += w(bit); then
// bitsPerByte*spb zeros.
struct FrameGen {
  double phase, w_mark, w_space;
  uint32_t pos;        // sample position inside the frame
  uint32_t frame_len;  // total samples
  uint32_t sig_begin, sig_end;  // [begin, end) carries tones
  uint32_t in_bit;     // samples emitted of the current bit
  uint32_t bit_idx;    // index of the current bit inside the frame
  uint32_t cur_bit;

  __device__ void start(const ModParams &M, double wm, double ws, uint32_t n_payload) {
    uint32_t total_bytes = M.n_pre + n_payload;
    uint32_t padding = total_bytes > 0 ? 2u * M.spb : 0u;
    phase = 0.0; w_mark = wm; w_space = ws;
    pos = 0;
    sig_begin = padding;
    sig_end = padding + total_bytes * M.bits_per_byte * M.spb;
    frame_len = sig_end + M.bits_per_byte * M.spb;
    in_bit = M.spb;  // forces a bit fetch at the first tone sample
    bit_idx = 0xFFFFFFFFu;
    cur_bit = 0;
  }
};

template <typename ByteFn>
__device__ inline uint32_t frame_bit(const ModParams &M, uint32_t bit_idx, ByteFn payload_byte) {
  uint32_t byte_i = bit_idx / M.bits_per_byte;
  uint32_t p = bit_idx - byte_i * M.bits_per_byte;
  uint32_t byte = byte_i < M.n_pre ? (uint32_t)M.pre[byte_i] : (uint32_t)payload_byte(byte_i - M.n_pre);
  if (p < M.start_bits) return 0u;
  p -= M.start_bits;
  if (p < 8u) return (byte >> (7u - p)) & 1u;
  p -= 8u;
  if (M.parity != 0u) {
    if (p == 0u) {
      uint32_t par = __builtin_popcount(byte & 0xFFu) & 1u;
      return M.parity == 1u ? par : 1u - par;
    }
    p -= 1u;
  }
  return 1u;  // stop bits
}

// Math.sin(phase) as the reference's engine computes it (fsk_fdlibm.h), rounded to f32 like the Float32Array store
__device__ inline double ref_sin(double phase) {
  bool exact;
  double sv = fdlibm::sin_medium(phase, &exact);
  if (!exact) sv = sin(phase);  // high word > 0x413921fb (2^20 * pi/2 rad): device library (see fsk_fdlibm.h)
  return sv;
}

// next sample of the frame (f32 like the Float32Array store, fsk.ts:403)
template <typename ByteFn>
__device__ inline float frame_next(FrameGen &G, const ModParams &M, ByteFn payload_byte) {
  float v = 0.0f;
  if (G.pos >= G.sig_begin && G.pos < G.sig_end) {
    if (G.in_bit == M.spb) {
      G.in_bit = 0;
      G.bit_idx++;
      G.cur_bit = frame_bit(M, G.bit_idx, payload_byte);
    }
    v = (float)sin(G.phase);  // (synthetic workload generator: device library sin)
    G.phase += G.cur_bit ? G.w_mark : G.w_space;
    G.in_bit++;
  }
  G.pos++;
  return v;
}

// Four consecutive samples.  The sequential part -- bit boundaries and the phase accumulation, in the reference's order
// of additions -- runs first; the four sines, which are independent of each other, are then evaluated as one
// straight-line block so their dependent chains overlap (one lane per stream means there is no other parallelism to
// hide an f64 polynomial behind).  en[j] = false leaves sample j untouched (0 returned, generator not advanced).
template <int N, bool EXACT, typename ByteFn>
__device__ inline void frame_next_block(FrameGen &G, const ModParams &M, ByteFn payload_byte, uint32_t en_mask, float *out) {
  double ph[N];
  bool tone[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    tone[j] = false;
    ph[j] = 4.0;  // any value of the straight-line case; unused unless tone[j]
    if (((en_mask >> j) & 1u) && G.pos < G.frame_len) {
      if (G.pos >= G.sig_begin && G.pos < G.sig_end) {
        if (G.in_bit == M.spb) {
          G.in_bit = 0;
          G.bit_idx++;
          G.cur_bit = frame_bit(M, G.bit_idx, payload_byte);
        }
        tone[j] = true;
        ph[j] = G.phase;
        G.phase += G.cur_bit ? G.w_mark : G.w_space;
        G.in_bit++;
      }
      G.pos++;
    }
  }
  double sv[N];
  if (EXACT) {
    bool slow[N];
    bool any_slow = false;
#pragma unroll
    for (int j = 0; j < N; j++) {
      sv[j] = fdlibm::sin_straight(ph[j], &slow[j]);
      any_slow |= slow[j] & tone[j];
    }
    if (__builtin_amdgcn_ballot_w64(any_slow)) {
#pragma unroll
      for (int j = 0; j < N; j++)
        if (slow[j] & tone[j]) sv[j] = ref_sin(ph[j]);  // first samples of a frame (phase < 3pi/4), near-multiples of pi/2, ...
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; j++) sv[j] = sin(ph[j]);
  }
#pragma unroll
  for (int j = 0; j < N; j++) out[j] = tone[j] ? (float)sv[j] : 0.0f;
}
template <bool EXACT, typename ByteFn>
__device__ inline float4 frame_next4(FrameGen &G, const ModParams &M, ByteFn payload_byte, bool e0, bool e1, bool e2,
                                     bool e3) {
  float o[4];
  frame_next_block<4, EXACT>(G, M, payload_byte, (e0 ? 1u : 0u) | (e1 ? 2u : 0u) | (e2 ? 4u : 0u) | (e3 ? 8u : 0u), o);
  return make_float4(o[0], o[1], o[2], o[3]);
}

// coalesced store of a 64-row x 32-sample LDS tile (rows = this wave's streams)
__device__ inline void store_tile(const float4 *stage, float *out, size_t pitch, size_t t0, size_t row_len_limit,
                                  uint32_t n_streams, const uint32_t *row_lens_lds, int vec_ok, uint32_t lane = 0xFFFFFFFFu) {
  if (lane == 0xFFFFFFFFu) lane = threadIdx.x;      // (one-wave blocks; modulate_wide_kernel passes the lane of its storing wave)
  const uint32_t sub_row = lane / kChunks, chunk = lane % kChunks;
#pragma unroll
  for (int i = 0; i < kChunks; i++) {
    uint32_t lr = (uint32_t)kRowsPerLoad * i + sub_row;
    uint32_t r = blockIdx.x * 64u + lr;
    if (r >= n_streams) continue;
    size_t lim = row_lens_lds ? (size_t)row_lens_lds[lr] : row_len_limit;
    size_t c0 = t0 + 4u * chunk;
    if (c0 >= lim) continue;
    float4 v = stage[chunk * kSlotStride + lr];
    float *dst = out + (size_t)r * pitch + c0;
    if (vec_ok && c0 + 4 <= lim) {
      *reinterpret_cast<float4 *>(dst) = v;
    } else {
      dst[0] = v.x;
      if (c0 + 1 < lim) dst[1] = v.y;
      if (c0 + 2 < lim) dst[2] = v.z;
      if (c0 + 3 < lim) dst[3] = v.w;
    }
  }
}

// modulateData for every stream: payloads [n_streams][payload_pitch] bytes, lens[s] bytes used.
template <bool EXACT>
__global__ __launch_bounds__(64) void modulate_kernel(ModParams M, const double *__restrict__ coef,
                                                      const uint8_t *__restrict__ payloads,
                                                      const uint32_t *__restrict__ lens, size_t payload_pitch,
                                                      float *__restrict__ out, size_t out_pitch, int vec_ok,
                                                      uint32_t *__restrict__ out_lens) {
  __shared__ float4 stage[kChunks * kSlotStride];
  __shared__ uint32_t row_len[64];
  __shared__ uint32_t max_len_s;
  const uint32_t lane = threadIdx.x;
  const uint32_t stream = blockIdx.x * 64u + lane;
  const bool valid = stream < M.n_streams;
  const uint32_t row = valid ? stream : M.n_streams - 1;
  const size_t ns = M.n_streams;
  const uint32_t n_payload = lens[row];
  const uint8_t *prow = payloads + (size_t)row * payload_pitch;
  auto pb = [&](uint32_t i) -> uint8_t { return prow[i]; };

  FrameGen G;
  G.start(M, coef[(size_t)CF_mark_w * ns + row], coef[(size_t)CF_space_w * ns + row], n_payload);
  uint32_t my_len = G.frame_len;
  if ((size_t)my_len > out_pitch) my_len = (uint32_t)out_pitch;  // caller reports overflow from out_lens
  row_len[lane] = valid ? my_len : 0u;
  if (valid) out_lens[stream] = G.frame_len;
  uint32_t mx = my_len;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { uint32_t t = __shfl_xor(mx, o, 64); mx = t > mx ? t : mx; }
  if (lane == 0) max_len_s = mx;
  __syncthreads();
  const uint32_t max_len = max_len_s;

  float *stage_f = reinterpret_cast<float *>(stage);
  for (uint32_t t0 = 0; t0 < max_len; t0 += kTile) {
    __syncthreads();
    for (uint32_t c = 0; c < (uint32_t)kChunks; c += 2) {   // eight sines per straight-line block
      float o[8];
      frame_next_block<8, EXACT>(G, M, pb, 0xFFu, o);
      stage[c * kSlotStride + lane] = make_float4(o[0], o[1], o[2], o[3]);
      stage[(c + 1) * kSlotStride + lane] = make_float4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
    store_tile(stage, out, out_pitch, t0, 0, M.n_streams, row_len, vec_ok);
  }
  (void)stage_f;
}

// ---- modulateData, several waves per 64-stream group (round 5) -----------------------------------------------------------
// modulate_kernel above is one wave per 64 streams, and what it spends its time on is not the sine: every sample goes through
// three nested per-lane conditionals (inside the frame? inside the tones? a new bit?), which compile to exec-mask branches
// of ~35 cycles each for a lone wave -- ~250 of the ~300 cycles a sample takes -- and 16 384 streams are 256 waves on 1 024
// SIMDs.  Here the control is UNIFORM: all streams of a call share samplesPerBit and start together, so sample positions, bit
// boundaries and tile boundaries are scalars; per lane there is only the bit's value, the end of the lane's own tones (payload
// lengths may differ) and the phase.  A tile is 32 samples; with samplesPerBit >= 32 it holds at most one bit boundary, so the
// phase chain of a tile is 32 x {w = (j >= jb ? w_next : w_cur), masked by "this lane still has tones"; ph[j] = phase; phase +=
// w} -- the reference's additions in the reference's order, straight-line.  ONE wave of the workgroup, the chain wave, runs
// that chain for every tile (it is the only sequential part: one f64 addition per sample, plus the bits' values) and hands
// every tile's start phase and its two increments per lane to the six owner waves through an LDS ring; the owner of a tile
// -- tile index mod 6 -- repeats the tile's 32 additions from that start phase (the same operations on the same operands),
// evaluates the 32 sines, which are independent, and stores the tile.  Values are those of modulate_kernel bit for bit.
static constexpr int kModWaves = 7;     // one chain wave + six owner waves (6 x 8 320 B of staging tiles + the hand-off ring: under 64 KB of static LDS)
static constexpr int kModOwners = kModWaves - 1;
static constexpr int kModRing = kModOwners;       // tiles of (start phase, w, w after the bit boundary) per lane between the chain wave and the owners
template <bool EXACT>
__global__ __launch_bounds__(64 * kModWaves) void modulate_wide_kernel(ModParams M, const double *__restrict__ coef,
                                                                       const uint8_t *__restrict__ payloads,
                                                                       const uint32_t *__restrict__ lens, size_t payload_pitch,
                                                                       float *__restrict__ out, size_t out_pitch, int vec_ok,
                                                                       uint32_t *__restrict__ out_lens) {
  __shared__ float4 stage_all[kModOwners][kChunks * kSlotStride];
  __shared__ double hand[kModRing][3][64];
  __shared__ uint32_t row_len[64];
  __shared__ uint32_t max_len_s;
  __shared__ uint32_t mctr[16];                                       // [0] tiles the chain wave has published, [1 + o] tiles owner o has taken
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t stream = blockIdx.x * 64u + lane;
  const bool valid = stream < M.n_streams;
  const uint32_t row = valid ? stream : M.n_streams - 1;
  const size_t ns = M.n_streams;
  const uint32_t n_payload = lens[row];
  const uint8_t *prow = payloads + (size_t)row * payload_pitch;
  const double wm = coef[(size_t)CF_mark_w * ns + row], ws = coef[(size_t)CF_space_w * ns + row];
  const uint32_t spb = M.spb;
  const uint32_t total_bytes = M.n_pre + n_payload;
  const uint32_t n_bits = total_bytes * M.bits_per_byte;            // this lane's tone bits
  const uint32_t sig_begin = 2u * spb;                               // (lanes with nothing to send have no tones: n_bits = 0)
  const uint32_t sig_end = total_bytes ? sig_begin + n_bits * spb : 0u;
  const uint32_t frame_len = sig_end + M.bits_per_byte * spb;        // fsk.ts:391-394
  uint32_t my_len = frame_len;
  if ((size_t)my_len > out_pitch) my_len = (uint32_t)out_pitch;      // caller reports overflow from out_lens
  if (threadIdx.x < 16) mctr[threadIdx.x] = 0;
  if (q == 0) {
    row_len[lane] = valid ? my_len : 0u;
    if (valid) out_lens[stream] = frame_len;
    uint32_t mx = my_len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { uint32_t t = __shfl_xor(mx, o, 64); mx = t > mx ? t : mx; }
    if (lane == 0) max_len_s = mx;
  }
  __syncthreads();
  const uint32_t max_len = max_len_s;
  const uint32_t n_tiles = (max_len + (uint32_t)kTile - 1u) / (uint32_t)kTile;
  FSK_WAIT_DECL
  auto peek = [&](const uint32_t *p) -> uint32_t {
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"((uint32_t)(uintptr_t)p) : "memory");
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
  };
  auto post = [&](uint32_t *p, uint32_t v) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\tds_write_b32 %0, %1" : : "v"((uint32_t)(uintptr_t)p), "v"(v) : "memory");
  };
  // One tile's phases from its start phase: the reference's additions in the reference's order (fsk.ts:404), straight-line; jb =
  // first sample of the tile in the next bit (>= kTile: none), rel = position of the tile's sample 0 inside the tones.  The chain
  // wave runs it for every tile (for the phase it hands on), an owner for its own tiles (for the 32 phases): the same operations
  // on the same operands, so the same values.
  auto tile_phases = [&](double phase, double w_cur, double w_next, uint32_t t0, int32_t rel, int32_t jb, double (&ph)[kTile], uint32_t &tone) -> double {
    tone = 0u;
#pragma unroll
    for (int j = 0; j < kTile; j++) {
      const bool in_tones = rel + j >= 0;                             // uniform
      const bool act = in_tones && (t0 + (uint32_t)j) < sig_end;
      const double wsel = j >= jb ? w_next : w_cur;                   // uniform choice between two per-lane values
      const double wj = act ? wsel : 0.0;
      ph[j] = phase;
      phase = phase + wj;                                             // (adding +0.0 outside the tones leaves it as it is)
      tone |= act ? (1u << j) : 0u;
    }
    return phase;
  };
  if (q == 0) {
    // ---------------------------------------------------------------- the chain wave: bit values, the phase at every tile's start
    // payload bytes one byte AHEAD of their use (bits are asked for in order: the byte index only ever moves on by one)
    uint32_t pay_idx = 0;
    uint32_t pay_cur = n_payload > 0u ? prow[0] : 0u, pay_nxt = n_payload > 1u ? prow[1] : 0u;
    auto pb = [&](uint32_t i) -> uint8_t {
      if (i != pay_idx) {                                             // (i == pay_idx + 1)
        pay_cur = pay_nxt; pay_idx = i;
        pay_nxt = i + 1u < n_payload ? prow[i + 1u] : 0u;
      }
      return (uint8_t)pay_cur;
    };
    auto w_of_bit = [&](uint32_t b) -> double {                       // phase increment of tone bit b of this lane (0 beyond its tones)
      uint32_t bit = 0u;
      if (b < n_bits) bit = frame_bit(M, b, pb);
      return b < n_bits ? (bit ? wm : ws) : 0.0;
    };
    double phase = 0.0, w_cur = 0.0;
    uint32_t b_have = 0xFFFFFFFFu;                                     // the bit w_cur belongs to (uniform)
    for (uint32_t tile = 0; tile < n_tiles; tile++) {
      const uint32_t t0 = tile * (uint32_t)kTile;
      const int32_t rel = (int32_t)t0 - (int32_t)sig_begin;
      double w_next = 0.0;
      int32_t jb = kTile;
      const bool tones = rel + (int32_t)kTile > 0;
      if (tones) {
        const uint32_t r0 = rel > 0 ? (uint32_t)rel : 0u;
        const uint32_t b0 = r0 / spb;                                 // bit of the tile's first tone sample
        if (b0 != b_have) { w_cur = w_of_bit(b0); b_have = b0; }
        jb = (int32_t)((b0 + 1u) * spb) - rel;
        if (jb < (int32_t)kTile) w_next = w_of_bit(b0 + 1u);
      }
      // the slot of tile - kModRing belongs to the same owner: it must have taken that one
      if (tile >= (uint32_t)kModRing) {
        const uint32_t o = tile % (uint32_t)kModOwners;
        FSK_WAIT_BEGIN
        while (peek(&mctr[1u + o]) + (uint32_t)kModRing <= tile) FSK_SPIN(1, M.stat);
      }
      double *h = &hand[tile % (uint32_t)kModRing][0][0];
      h[lane] = phase; h[64 + lane] = w_cur; h[128 + lane] = w_next;
      post(&mctr[0], tile + 1u);
      if (tones) {
        double ph[kTile];
        uint32_t tone;
        phase = tile_phases(phase, w_cur, w_next, t0, rel, jb, ph, tone);
        if (jb < (int32_t)kTile) { w_cur = w_next; b_have = (uint32_t)(((rel > 0 ? (uint32_t)rel : 0u) / spb) + 1u); }
      }
    }
    return;
  }
  // ------------------------------------------------------------------ an owner wave: every kModOwners-th tile -- its 32 sines, transposed through LDS, stored
  const uint32_t o = q - 1u;
  float4 *stage = stage_all[o];
  for (uint32_t tile = o; tile < n_tiles; tile += (uint32_t)kModOwners) {
    const uint32_t t0 = tile * (uint32_t)kTile;
    const int32_t rel = (int32_t)t0 - (int32_t)sig_begin;
    FSK_WAIT_BEGIN
    while (peek(&mctr[0]) <= tile) FSK_SPIN(1, M.stat);
    const double *h = &hand[tile % (uint32_t)kModRing][0][0];
    const double phase0 = h[lane], w_cur = h[64 + lane], w_next = h[128 + lane];
    post(&mctr[1u + o], tile + 1u);                                   // (taken: the chain wave may reuse the slot)
    double ph[kTile];
    uint32_t tone = 0u;
    if (rel + (int32_t)kTile > 0) {
      const uint32_t r0 = rel > 0 ? (uint32_t)rel : 0u;
      const int32_t jb = (int32_t)((r0 / spb + 1u) * spb) - rel;
      (void)tile_phases(phase0, w_cur, w_next, t0, rel, jb, ph, tone);
    }
    if (__builtin_amdgcn_ballot_w64(tone != 0u) == 0ull) {          // padding: zeros (fsk.ts:391-396)
#pragma unroll
      for (int c = 0; c < kChunks; c++) stage[c * kSlotStride + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
      for (int c = 0; c < kChunks; c += 2) {
        float ov[8];
        double sv[8], p8[8];
        bool tn[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          tn[j] = ((tone >> (4 * c + j)) & 1u) != 0u;
          p8[j] = tn[j] ? ph[4 * c + j] : 4.0;                          // (any value of the straight-line case where there is no tone)
        }
        if (EXACT) {
          bool slow[8];
          bool any_slow = false;
#pragma unroll
          for (int j = 0; j < 8; j++) {
            sv[j] = fdlibm::sin_straight(p8[j], &slow[j]);
            any_slow |= slow[j] & tn[j];
          }
          if (__builtin_amdgcn_ballot_w64(any_slow)) {
#pragma unroll
            for (int j = 0; j < 8; j++)
              if (slow[j] & tn[j]) sv[j] = ref_sin(p8[j]);              // first samples of a frame (phase < 3pi/4), near-multiples of pi/2, ...
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) sv[j] = sin(p8[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) ov[j] = tn[j] ? (float)sv[j] : 0.0f;
        stage[c * kSlotStride + lane] = make_float4(ov[0], ov[1], ov[2], ov[3]);
        stage[(c + 1) * kSlotStride + lane] = make_float4(ov[4], ov[5], ov[6], ov[7]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                // (one wave: its own writes, in order)
    store_tile(stage, out, out_pitch, t0, 0, M.n_streams, row_len, vec_ok, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// synthetic workload: see fskhip_synth_device in include/fskhip.h
__global__ __launch_bounds__(64) void synth_kernel(ModParams M, const double *__restrict__ coef,
                                                   float *__restrict__ out, size_t n, size_t pitch, int vec_ok,
                                                   uint32_t payload_len, uint64_t seed, uint32_t lead_max,
                                                   double amp_lo, double amp_hi) {
  __shared__ float4 stage[kChunks * kSlotStride];
  const uint32_t lane = threadIdx.x;
  const uint32_t stream = blockIdx.x * 64u + lane;
  const bool valid = stream < M.n_streams;
  const uint32_t row = valid ? stream : M.n_streams - 1;
  const size_t ns = M.n_streams;
  const double wm = coef[(size_t)CF_mark_w * ns + row], ws = coef[(size_t)CF_space_w * ns + row];

  uint32_t lead;
  double amp;
  synth_stream_params(seed, row, lead_max, amp_lo, amp_hi, &lead, &amp);
  uint32_t frame = 0;
  auto pb = [&](uint32_t i) -> uint8_t { return synth_payload_byte(seed, row, frame, i); };
  FrameGen G;
  G.start(M, wm, ws, payload_len);
  uint64_t t = 0;  // absolute sample index

  auto next = [&]() -> float {
    float v = 0.0f;
    if (t >= lead) {
      if (G.pos >= G.frame_len) { frame++; G.start(M, wm, ws, payload_len); }
      float s = frame_next(G, M, pb);
      v = (float)((double)s * amp);
    }
    t++;
    return v;
  };

  for (size_t t0 = 0; t0 < n; t0 += kTile) {
    __syncthreads();
    for (uint32_t c = 0; c < (uint32_t)kChunks; c++) {
      float4 v;
      v.x = next(); v.y = next(); v.z = next(); v.w = next();
      stage[c * kSlotStride + lane] = v;
    }
    __syncthreads();
    store_tile(stage, out, pitch, t0, n, M.n_streams, nullptr, vec_ok);
  }
}

// ---- FSKProcessor.process() for every stream ------------------------------------------------------
// One launch per quantum after the demodulator: (1) processDemodulation's ring puts (fsk-processor.ts:310-318,
// utils.ts:38-48) of the bytes the demod kernels just produced, (2) modulateTo (256-276): zero fill, then the next
// n_out samples of the pending modulation from its generator state, completion bookkeeping, and optionally the RX
// clear the 'modulate' handler does when the modulation resolves (228-235).
template <bool EXACT>
__global__ __launch_bounds__(64) void processor_io_kernel(ModParams M, const double *__restrict__ coef, ProcState T,
                                                          const uint8_t *__restrict__ demod_out, size_t demod_pitch,
                                                          const uint32_t *__restrict__ demod_counts, int do_rx,
                                                          float *__restrict__ out, size_t n_out, size_t out_pitch,
                                                          int vec_ok, uint32_t clear_rx_on_complete) {
  __shared__ float4 stage[kChunks * kSlotStride];
  const uint32_t lane = threadIdx.x;
  const uint32_t stream = blockIdx.x * 64u + lane;
  const bool valid = stream < M.n_streams;
  const uint32_t row = valid ? stream : M.n_streams - 1;
  const size_t ns = M.n_streams;

  uint32_t w = T.rx_w[row], r = T.rx_r[row], len = T.rx_len[row];
  bool rx_dirty = false;
  if (do_rx && valid) {
    uint32_t cnt = demod_counts[stream];
    if ((size_t)cnt > demod_pitch) cnt = (uint32_t)demod_pitch;
    const uint8_t *src = demod_out + (size_t)stream * demod_pitch;
    uint8_t *ring = T.rx_buf + (size_t)stream * T.rx_cap;
    for (uint32_t i = 0; i < cnt; i++) {  // put(): overwrite the oldest when full
      ring[w] = src[i];
      w = w + 1 == T.rx_cap ? 0u : w + 1;
      if (len < T.rx_cap) len++;
      else r = r + 1 == T.rx_cap ? 0u : r + 1;
    }
    rx_dirty = cnt != 0;
  }

  if (out != nullptr && n_out > 0) {
    const uint32_t flen = T.tx_len[row];
    const bool active = valid && T.tx_pending[row] != 0u && flen > 0u && T.tx_pos[row] < flen;
    const uint8_t *prow = T.tx_payload + (size_t)row * T.tx_payload_pitch;
    auto pb = [&](uint32_t i) -> uint8_t { return prow[i]; };
    FrameGen G;
    G.start(M, coef[(size_t)CF_mark_w * ns + row], coef[(size_t)CF_space_w * ns + row], T.tx_n_payload[row]);
    if (active) {
      G.phase = T.tx_phase[row]; G.pos = T.tx_pos[row]; G.in_bit = T.tx_in_bit[row];
      G.bit_idx = T.tx_bit_idx[row]; G.cur_bit = T.tx_cur_bit[row];
    } else {
      G.pos = G.frame_len;  // nothing to emit: zeros
    }
    for (size_t t0 = 0; t0 < n_out; t0 += kTile) {
      __syncthreads();
      for (uint32_t c = 0; c < (uint32_t)kChunks; c++) {
        // samples beyond n_out inside the last tile must not advance the generator
        const size_t base = t0 + 4u * c;
        stage[c * kSlotStride + lane] = frame_next4<EXACT>(G, M, pb, base + 0 < n_out, base + 1 < n_out, base + 2 < n_out, base + 3 < n_out);
      }
      __syncthreads();
      store_tile(stage, out, out_pitch, t0, n_out, M.n_streams, nullptr, vec_ok);
    }
    if (active) {
      if (G.pos >= flen) {  // isComplete: ChunkedModulator.reset() + pendingModulation = null
        T.tx_pos[stream] = 0u; T.tx_len[stream] = 0u; T.tx_pending[stream] = 0u;
        T.tx_completed[stream] += 1u;
        if (clear_rx_on_complete) { w = 0u; r = 0u; len = 0u; rx_dirty = true; }
      } else {
        T.tx_phase[stream] = G.phase; T.tx_pos[stream] = G.pos; T.tx_in_bit[stream] = G.in_bit;
        T.tx_bit_idx[stream] = G.bit_idx; T.tx_cur_bit[stream] = G.cur_bit;
      }
    }
  }
  if (rx_dirty && valid) { T.rx_w[stream] = w; T.rx_r[stream] = r; T.rx_len[stream] = len; }
}

// The packed code rows of one tile of a one-wave workgroup -- row lr: the kTile codes of stream blockIdx.x * 64 + lr from column t0
// on, rows kTile * sizeof(Bits) / 4 + 1 words apart -- stored to the stream-major `out`: as 16-byte vectors, 16 / 32 rows of
// 64 / 32 contiguous bytes per instruction (16-bit / G.711), or -- where the base or the pitch is off the 16-byte grid (vec_ok = 0)
// -- as single elements, two rows of 32 consecutive ones per instruction.  Nothing is written from column n_out or row n_streams on.
template <typename Bits>
__device__ __forceinline__ void store_code_rows(const uint32_t *codes, Bits *out, size_t out_pitch, size_t t0, size_t n_out, uint32_t n_streams, int vec_ok,
                                                uint32_t lane) {
  constexpr uint32_t kEsz = (uint32_t)sizeof(Bits);
  constexpr uint32_t kWords = (uint32_t)kTile * kEsz / 4u, kRowPitch = kWords + 1u;
  constexpr uint32_t kVecEls = 16u / kEsz;                      // elements of a 16-byte vector
  if (vec_ok) {
    constexpr uint32_t kLanesPerRow = kWords / 4u, kRowsPerStore = 64u / kLanesPerRow;
    const uint32_t sub_row = lane / kLanesPerRow, q = lane % kLanesPerRow;
#pragma unroll
    for (uint32_t i = 0; i < kLanesPerRow; i++) {
      const uint32_t lr = kRowsPerStore * i + sub_row;
      const uint32_t rr = blockIdx.x * 64u + lr;
      const size_t c0 = t0 + (size_t)kVecEls * q;
      if (rr >= n_streams || c0 >= n_out) continue;
      const uint32_t *src = &codes[lr * kRowPitch + 4u * q];
      Bits *dst = out + (size_t)rr * out_pitch + c0;
      if (c0 + kVecEls <= n_out) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(src[0], src[1], src[2], src[3]);
      } else {   // the row's last, partial vector
        for (uint32_t e = 0; c0 + e < n_out; e++) dst[e] = (Bits)(src[e * kEsz / 4u] >> (8u * ((e * kEsz) & 3u)));
      }
    }
  } else {
    const uint32_t half = lane >> 5, e = lane & 31u;
    const size_t col = t0 + e;
#pragma unroll 4
    for (uint32_t i = 0; i < 32u; i++) {
      const uint32_t lr = 2u * i + half;
      const uint32_t rr = blockIdx.x * 64u + lr;
      if (rr < n_streams && col < n_out) out[(size_t)rr * out_pitch + col] = (Bits)(codes[lr * kRowPitch + e * kEsz / 4u] >> (8u * ((e * kEsz) & 3u)));
    }
  }
}

// The same quantum with the output in a capture format and layout (fskhip_processor_process_fmt_*; FMT / LAYOUT: include/fskhip.h's
// FSKHIP_SAMPLES_* / FSKHIP_LAYOUT_*): processor_io_kernel's bookkeeping and generator, statement for statement, and behind the
// generator SampleFmt<FMT>::encode -- element (s, t) of `out_` is the code of the float that kernel writes there, its zero fill the
// format's silence.  The codes leave the registers for `out_` themselves: no float tile in HBM, no second launch.
//   sample-major   [sample][channel] frames: a lane is a stream, so a wave instruction stores 64 consecutive elements of one frame;
//                  columns from n_streams on are not written.
//   stream-major   the lane packs its row's 32 codes of a tile into kTile * sizeof(element) / 4 words of LDS (rows an odd number of
//                  words apart: every bank once per half wave); the wave then stores them as 16-byte vectors, 16 / 32 rows of
//                  64 / 32 contiguous bytes per instruction (16-bit / G.711), or -- where the base or the pitch is off the 16-byte
//                  grid (vec_ok = 0) -- as single elements, two rows of 32 consecutive ones per instruction.  float32 in this layout
//                  is processor_io_kernel itself.
template <bool EXACT, int FMT, int LAYOUT>
__global__ __launch_bounds__(64) void processor_io_fmt_kernel(ModParams M, const double *__restrict__ coef, ProcState T,
                                                              const uint8_t *__restrict__ demod_out, size_t demod_pitch,
                                                              const uint32_t *__restrict__ demod_counts, int do_rx,
                                                              void *__restrict__ out_, size_t n_out, size_t out_pitch,
                                                              int vec_ok, uint32_t clear_rx_on_complete) {
  static_assert(FMT != FSKHIP_SAMPLES_F32 || LAYOUT != FSKHIP_LAYOUT_STREAM_MAJOR, "float32 stream-major is processor_io_kernel");
  using F = SampleFmt<FMT>;
  const uint32_t lane = threadIdx.x;
  const uint32_t stream = blockIdx.x * 64u + lane;
  const bool valid = stream < M.n_streams;
  const uint32_t row = valid ? stream : M.n_streams - 1;
  const size_t ns = M.n_streams;

  uint32_t w = T.rx_w[row], r = T.rx_r[row], len = T.rx_len[row];
  bool rx_dirty = false;
  if (do_rx && valid) {
    uint32_t cnt = demod_counts[stream];
    if ((size_t)cnt > demod_pitch) cnt = (uint32_t)demod_pitch;
    const uint8_t *src = demod_out + (size_t)stream * demod_pitch;
    uint8_t *ring = T.rx_buf + (size_t)stream * T.rx_cap;
    for (uint32_t i = 0; i < cnt; i++) {  // put(): overwrite the oldest when full
      ring[w] = src[i];
      w = w + 1 == T.rx_cap ? 0u : w + 1;
      if (len < T.rx_cap) len++;
      else r = r + 1 == T.rx_cap ? 0u : r + 1;
    }
    rx_dirty = cnt != 0;
  }

  if (out_ != nullptr && n_out > 0) {
    const uint32_t flen = T.tx_len[row];
    const bool active = valid && T.tx_pending[row] != 0u && flen > 0u && T.tx_pos[row] < flen;
    const uint8_t *prow = T.tx_payload + (size_t)row * T.tx_payload_pitch;
    auto pb = [&](uint32_t i) -> uint8_t { return prow[i]; };
    FrameGen G;
    G.start(M, coef[(size_t)CF_mark_w * ns + row], coef[(size_t)CF_space_w * ns + row], T.tx_n_payload[row]);
    if (active) {
      G.phase = T.tx_phase[row]; G.pos = T.tx_pos[row]; G.in_bit = T.tx_in_bit[row];
      G.bit_idx = T.tx_bit_idx[row]; G.cur_bit = T.tx_cur_bit[row];
    } else {
      G.pos = G.frame_len;  // nothing to emit: zeros
    }
    typename F::Bits *const out = (typename F::Bits *)out_;
    constexpr uint32_t kEsz = (uint32_t)sizeof(typename F::Bits);
    constexpr uint32_t kWords = (uint32_t)kTile * kEsz / 4u;          // words of codes per row of a tile
    constexpr uint32_t kRowPitch = kWords + 1u;                       // odd
    __shared__ uint32_t codes[LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR ? 64u * kRowPitch : 1u];
    for (size_t t0 = 0; t0 < n_out; t0 += kTile) {
      if constexpr (LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR) __syncthreads();   // (the tile's readers of the round before)
      for (uint32_t c = 0; c < (uint32_t)kChunks; c++) {
        const size_t base = t0 + 4u * c;
        const float4 v = frame_next4<EXACT>(G, M, pb, base + 0 < n_out, base + 1 < n_out, base + 2 < n_out, base + 3 < n_out);
        const float o[4] = {v.x, v.y, v.z, v.w};
        uint32_t k[4];
#pragma unroll
        for (int j = 0; j < 4; j++) k[j] = F::encode(o[j]);
        if constexpr (LAYOUT == FSKHIP_LAYOUT_SAMPLE_MAJOR) {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (valid && base + j < n_out) out[(base + j) * out_pitch + stream] = (typename F::Bits)k[j];
        } else if constexpr (kEsz == 2) {
          codes[lane * kRowPitch + 2u * c] = k[0] | (k[1] << 16);
          codes[lane * kRowPitch + 2u * c + 1u] = k[2] | (k[3] << 16);
        } else {
          codes[lane * kRowPitch + c] = k[0] | (k[1] << 8) | (k[2] << 16) | (k[3] << 24);
        }
      }
      if constexpr (LAYOUT == FSKHIP_LAYOUT_STREAM_MAJOR) {
        __syncthreads();
        store_code_rows(codes, out, out_pitch, t0, n_out, M.n_streams, vec_ok, lane);
      }
    }
    if (active) {
      if (G.pos >= flen) {  // isComplete: ChunkedModulator.reset() + pendingModulation = null
        T.tx_pos[stream] = 0u; T.tx_len[stream] = 0u; T.tx_pending[stream] = 0u;
        T.tx_completed[stream] += 1u;
        if (clear_rx_on_complete) { w = 0u; r = 0u; len = 0u; rx_dirty = true; }
      } else {
        T.tx_phase[stream] = G.phase; T.tx_pos[stream] = G.pos; T.tx_in_bit[stream] = G.in_bit;
        T.tx_bit_idx[stream] = G.bit_idx; T.tx_cur_bit[stream] = G.cur_bit;
      }
    }
  }
  if (rx_dirty && valid) { T.rx_w[stream] = w; T.rx_r[stream] = r; T.rx_len[stream] = len; }
}

// The same quantum with the output at a decimator's low rate (fskhip_processor_process_rate_*): processor_io_kernel's bookkeeping and
// generator, statement for statement, over n_out * Ld samples that never reach HBM, and behind the generator resample_down_kernel's
// sum (fsk_resample.hip: y[k] = f32(sum_i c[i] u[kL - i]), i ascending, `mac` in the handle's precision) and SampleFmt<FMT>::encode.
// Lane = stream; the workgroup's one wave owns its 64 streams for the whole quantum.  The samples go into a delay line in LDS,
// [slot][lane] with rows kRateLanePitch words apart (fsk_processor_rate_plan.h): a tap is 64 consecutive words, a lane only ever
// reads and writes its own column, and the taps are wave-uniform (scalar loads).  The handle's history -- n_taps - 1 floats per
// stream, oldest first -- is read coalesced, 64 consecutive floats of one stream per instruction, into slots [0, n_taps - 1) at
// entry; the samples follow round the ring, kRateChunk per step of the generator, and every Ld-th one is an output, taken as soon
// as it is written.  At exit the last n_taps - 1 samples are written to hist_out the same way (the two history buffers ping-pong
// as the handle's own calls have them).  The codes leave stream-major as processor_io_fmt_kernel's do, through the packed code rows,
// kTile outputs per flush.  (Interleaved frames take the two launches this kernel replaces: written from the registers, 64
// consecutive elements of a frame per instruction, it measured 1.10 to 1.26 times that pair -- profiles/processor_rate_bench.jsonl.)
// The launcher has seen to n_out > 0, a delay line of `slots` >= n_taps - 1 + max(Ld, kRateChunk) samples and the LDS for it.
template <bool EXACT, typename Real, int FMT>
__global__ __launch_bounds__(64) void processor_io_rate_kernel(ModParams M, const double *__restrict__ coef, ProcState T,
                                                               const uint8_t *__restrict__ demod_out, size_t demod_pitch,
                                                               const uint32_t *__restrict__ demod_counts, int do_rx,
                                                               void *__restrict__ out_, size_t n_out, size_t out_pitch, int vec_ok,
                                                               uint32_t clear_rx_on_complete, const float *__restrict__ hist_in,
                                                               float *__restrict__ hist_out, const void *__restrict__ taps_, uint32_t Ld,
                                                               uint32_t n_taps, uint32_t slots) {
  using F = SampleFmt<FMT>;
  using Bits = typename F::Bits;
  static_assert(kRateCodeTile == (uint32_t)kTile && kRateChunk == 4u, "the code rows are store_code_rows', the generator's step frame_next4's");
  constexpr uint32_t kPitch = kRateLanePitch;
  constexpr uint32_t kRowPitch = (uint32_t)kTile * (uint32_t)sizeof(Bits) / 4u + 1u;
  extern __shared__ __align__(16) unsigned char rate_lds[];
  float *const dl = reinterpret_cast<float *>(rate_lds);               // [slots][kPitch]
  uint32_t *const codes = reinterpret_cast<uint32_t *>(dl + (size_t)slots * kPitch);   // [64][kRowPitch]
  const uint32_t lane = threadIdx.x;
  const uint32_t stream = blockIdx.x * 64u + lane;
  const bool valid = stream < M.n_streams;
  const uint32_t row = valid ? stream : M.n_streams - 1;
  const size_t ns = M.n_streams;

  uint32_t w = T.rx_w[row], r = T.rx_r[row], len = T.rx_len[row];
  bool rx_dirty = false;
  if (do_rx && valid) {
    uint32_t cnt = demod_counts[stream];
    if ((size_t)cnt > demod_pitch) cnt = (uint32_t)demod_pitch;
    const uint8_t *src = demod_out + (size_t)stream * demod_pitch;
    uint8_t *ring = T.rx_buf + (size_t)stream * T.rx_cap;
    for (uint32_t i = 0; i < cnt; i++) {  // put(): overwrite the oldest when full
      ring[w] = src[i];
      w = w + 1 == T.rx_cap ? 0u : w + 1;
      if (len < T.rx_cap) len++;
      else r = r + 1 == T.rx_cap ? 0u : r + 1;
    }
    rx_dirty = cnt != 0;
  }

  {
    const uint32_t flen = T.tx_len[row];
    const bool active = valid && T.tx_pending[row] != 0u && flen > 0u && T.tx_pos[row] < flen;
    const uint8_t *prow = T.tx_payload + (size_t)row * T.tx_payload_pitch;
    auto pb = [&](uint32_t i) -> uint8_t { return prow[i]; };
    FrameGen G;
    G.start(M, coef[(size_t)CF_mark_w * ns + row], coef[(size_t)CF_space_w * ns + row], T.tx_n_payload[row]);
    if (active) {
      G.phase = T.tx_phase[row]; G.pos = T.tx_pos[row]; G.in_bit = T.tx_in_bit[row];
      G.bit_idx = T.tx_bit_idx[row]; G.cur_bit = T.tx_cur_bit[row];
    } else {
      G.pos = G.frame_len;  // nothing to emit: zeros
    }
    Bits *const out = (Bits *)out_;
    const Real *const taps = (const Real *)taps_;
    const uint32_t H = n_taps - 1u;
    // the history: sample -H + h of the quantum at slot h; streams past the batch hold zeros
    for (uint32_t c = 0; c < 64u; c++) {
      const uint32_t s = blockIdx.x * 64u + c;
      for (uint32_t h = lane; h < H; h += 64u) dl[h * kPitch + c] = s < M.n_streams ? hist_in[(size_t)s * H + h] : 0.0f;
    }
    __syncthreads();
    const size_t n_high = n_out * Ld;
    uint32_t wslot = H;        // the slot of sample t0: (H + t0) mod slots
    uint32_t ph = 0;           // t mod Ld
    size_t k = 0;              // the next output
    for (size_t t0 = 0; t0 < n_high; t0 += kRateChunk) {
      // samples beyond n_high inside the last step must not advance the generator
      const float4 v = frame_next4<EXACT>(G, M, pb, t0 + 0 < n_high, t0 + 1 < n_high, t0 + 2 < n_high, t0 + 3 < n_high);
      const float o[4] = {v.x, v.y, v.z, v.w};
      const uint32_t cnt = n_high - t0 < kRateChunk ? (uint32_t)(n_high - t0) : kRateChunk;
      uint32_t sl = wslot;
#pragma unroll
      for (uint32_t j = 0; j < kRateChunk; j++) {
        if (j < cnt) {
          dl[sl * kPitch + lane] = o[j];
          sl = sl + 1u == slots ? 0u : sl + 1u;
        }
      }
      for (uint32_t j = 0; j < cnt; j++) {
        if (ph == 0u) {      // sample t0 + j = k Ld: output k, tap i at the slot i behind it
          uint32_t si = wslot + j;
          si = si >= slots ? si - slots : si;
          Real acc = 0;
#pragma unroll 8
          for (uint32_t i = 0; i < n_taps; i++) {
            acc = mac(acc, taps[i], dl[si * kPitch + lane]);
            si = si == 0u ? slots - 1u : si - 1u;
          }
          const uint32_t code = F::encode((float)acc);
          const uint32_t kk = (uint32_t)(k & (size_t)(kTile - 1));
          reinterpret_cast<Bits *>(codes + lane * kRowPitch)[kk] = (Bits)code;
          if (kk == (uint32_t)kTile - 1u || k + 1 == n_out) {
            __syncthreads();
            store_code_rows(codes, out, out_pitch, k - kk, n_out, M.n_streams, vec_ok, lane);
            __syncthreads();   // (the rows' readers, before the next tile's codes)
          }
          k++;
        }
        ph = ph + 1u == Ld ? 0u : ph + 1u;
      }
      wslot = sl;
    }
    // the history after the call: samples n_high - H + h, at slot (n_high + h) mod slots
    __syncthreads();
    const uint32_t hbase = (uint32_t)(n_high % slots);
    for (uint32_t c = 0; c < 64u; c++) {
      const uint32_t s = blockIdx.x * 64u + c;
      if (s >= M.n_streams) break;
      for (uint32_t h = lane; h < H; h += 64u) {
        uint32_t si = hbase + h;
        si = si >= slots ? si - slots : si;
        hist_out[(size_t)s * H + h] = dl[si * kPitch + c];
      }
    }
    if (active) {
      if (G.pos >= flen) {  // isComplete: ChunkedModulator.reset() + pendingModulation = null
        T.tx_pos[stream] = 0u; T.tx_len[stream] = 0u; T.tx_pending[stream] = 0u;
        T.tx_completed[stream] += 1u;
        if (clear_rx_on_complete) { w = 0u; r = 0u; len = 0u; rx_dirty = true; }
      } else {
        T.tx_phase[stream] = G.phase; T.tx_pos[stream] = G.pos; T.tx_in_bit[stream] = G.in_bit;
        T.tx_bit_idx[stream] = G.bit_idx; T.tx_cur_bit[stream] = G.cur_bit;
      }
    }
  }
  if (rx_dirty && valid) { T.rx_w[stream] = w; T.rx_r[stream] = r; T.rx_len[stream] = len; }
}

// The same quantum with the output behind a playback converter (fskhip_processor_process_ratecvt_*): the rational counterpart of
// processor_io_rate_kernel, in its shape -- one wave per 64 streams, lane = stream, processor_io_kernel's bookkeeping and generator
// statement for statement, the samples in the [slot][lane] delay line, the codes out through the packed code rows, the history read
// at entry and written at exit, coalesced.  The filter is ratecvt_playback_kernel's (fsk_ratecvt.hip) with up factor Lu and down
// factor Md: output j has phase p = (j Md) mod Lu and newest input m = (j Md) div Lu, both kept by wave-uniform integer
// accumulators, and is taken as soon as sample m is written -- one sample may complete none, one or several outputs.  Its sum is
// that kernel's: the k_full = n_taps / Lu products every phase has, k ascending, then the one more of a phase p < n_taps mod Lu,
// `mac` in the handle's precision, the taps from the [K][Lu] table in output order (column j mod Lu; wave-uniform, scalar loads) --
// the same float, bit for bit.  The handle's history is H = ceil((n_taps - 1) / Lu) samples per stream, and the sum reaches back at
// most H from m, so the delay line is H + kRateChunk slots (fsk_processor_rate_plan.h: processor_ratecvt_plan).
// Two forms of the one body.  !ANY is a quantum of whole periods from a period boundary: n_out a multiple of Lu, the accumulators
// start at zero and the quantum is n_out / Lu * Md samples; the four trailing arguments are not read.  ANY is a quantum of any n_out
// from the handle's position (fskhip_processor_process_ratecvt_any_*): the host passes where it starts on the period grid
// (fsk_processor_rate_plan.h: processor_ratecvt_start) -- n_high_any samples to generate, and the first output's tap column q0,
// phase ph0 and newest input m0 counted from the quantum's first sample, wave-uniform like everything the tap loads depend on.
// Output k0 + k of the grid is stored at column k.  The history at exit is the H newest samples in either form: a quantum of fewer
// than H samples leaves the rest of the old history, which still lies in the ring, in front of its own.
// The launcher has seen to n_out > 0 (!ANY: a multiple of Lu), `slots` >= H + kRateChunk and the LDS for it.
template <bool EXACT, typename Real, int FMT, bool ANY>
__global__ __launch_bounds__(64) void processor_io_ratecvt_kernel(ModParams M, const double *__restrict__ coef, ProcState T,
                                                                  const uint8_t *__restrict__ demod_out, size_t demod_pitch,
                                                                  const uint32_t *__restrict__ demod_counts, int do_rx,
                                                                  void *__restrict__ out_, size_t n_out, size_t out_pitch, int vec_ok,
                                                                  uint32_t clear_rx_on_complete, const float *__restrict__ hist_in,
                                                                  float *__restrict__ hist_out, const void *__restrict__ taps_, uint32_t Lu,
                                                                  uint32_t Md, uint32_t n_taps, uint32_t slots, size_t n_high_any,
                                                                  uint32_t q0, uint32_t ph0, uint32_t m0) {
  using F = SampleFmt<FMT>;
  using Bits = typename F::Bits;
  static_assert(kRateCodeTile == (uint32_t)kTile && kRateChunk == 4u, "the code rows are store_code_rows', the generator's step frame_next4's");
  constexpr uint32_t kPitch = kRateLanePitch;
  constexpr uint32_t kRowPitch = (uint32_t)kTile * (uint32_t)sizeof(Bits) / 4u + 1u;
  extern __shared__ __align__(16) unsigned char rate_lds[];
  float *const dl = reinterpret_cast<float *>(rate_lds);               // [slots][kPitch]
  uint32_t *const codes = reinterpret_cast<uint32_t *>(dl + (size_t)slots * kPitch);   // [64][kRowPitch]
  const uint32_t lane = threadIdx.x;
  const uint32_t stream = blockIdx.x * 64u + lane;
  const bool valid = stream < M.n_streams;
  const uint32_t row = valid ? stream : M.n_streams - 1;
  const size_t ns = M.n_streams;

  uint32_t w = T.rx_w[row], r = T.rx_r[row], len = T.rx_len[row];
  bool rx_dirty = false;
  if (do_rx && valid) {
    uint32_t cnt = demod_counts[stream];
    if ((size_t)cnt > demod_pitch) cnt = (uint32_t)demod_pitch;
    const uint8_t *src = demod_out + (size_t)stream * demod_pitch;
    uint8_t *ring = T.rx_buf + (size_t)stream * T.rx_cap;
    for (uint32_t i = 0; i < cnt; i++) {  // put(): overwrite the oldest when full
      ring[w] = src[i];
      w = w + 1 == T.rx_cap ? 0u : w + 1;
      if (len < T.rx_cap) len++;
      else r = r + 1 == T.rx_cap ? 0u : r + 1;
    }
    rx_dirty = cnt != 0;
  }

  {
    const uint32_t flen = T.tx_len[row];
    const bool active = valid && T.tx_pending[row] != 0u && flen > 0u && T.tx_pos[row] < flen;
    const uint8_t *prow = T.tx_payload + (size_t)row * T.tx_payload_pitch;
    auto pb = [&](uint32_t i) -> uint8_t { return prow[i]; };
    FrameGen G;
    G.start(M, coef[(size_t)CF_mark_w * ns + row], coef[(size_t)CF_space_w * ns + row], T.tx_n_payload[row]);
    if (active) {
      G.phase = T.tx_phase[row]; G.pos = T.tx_pos[row]; G.in_bit = T.tx_in_bit[row];
      G.bit_idx = T.tx_bit_idx[row]; G.cur_bit = T.tx_cur_bit[row];
    } else {
      G.pos = G.frame_len;  // nothing to emit: zeros
    }
    Bits *const out = (Bits *)out_;
    const Real *const taps = (const Real *)taps_;                      // [K][Lu], column q: the taps of output q of a period
    const uint32_t H = (n_taps - 1u + Lu - 1u) / Lu;
    const uint32_t k_full = n_taps / Lu, rem = n_taps - k_full * Lu;   // phase p has k_full + (p < rem) taps
    // the history: sample -H + h of the quantum at slot h; streams past the batch hold zeros
    for (uint32_t c = 0; c < 64u; c++) {
      const uint32_t s = blockIdx.x * 64u + c;
      for (uint32_t h = lane; h < H; h += 64u) dl[h * kPitch + c] = s < M.n_streams ? hist_in[(size_t)s * H + h] : 0.0f;
    }
    __syncthreads();
    const size_t n_high = ANY ? n_high_any : n_out / Lu * Md;
    uint32_t wslot = H;        // the slot of sample t0: (H + t0) mod slots
    size_t k = 0;              // the next output (ANY: output k0 + k of the period grid)
    uint32_t q = ANY ? q0 : 0u, ph = ANY ? ph0 : 0u;    // (k0 + k) mod Lu, ((k0 + k) Md) mod Lu
    size_t m = ANY ? m0 : 0u;  // ((k0 + k) Md) div Lu - pos: the sample that completes output k
    for (size_t t0 = 0; t0 < n_high; t0 += kRateChunk) {
      // samples beyond n_high inside the last step must not advance the generator
      const float4 v = frame_next4<EXACT>(G, M, pb, t0 + 0 < n_high, t0 + 1 < n_high, t0 + 2 < n_high, t0 + 3 < n_high);
      const float o[4] = {v.x, v.y, v.z, v.w};
      const uint32_t cnt = n_high - t0 < kRateChunk ? (uint32_t)(n_high - t0) : kRateChunk;
      uint32_t sl = wslot;
#pragma unroll
      for (uint32_t j = 0; j < kRateChunk; j++) {
        if (j < cnt) {
          dl[sl * kPitch + lane] = o[j];
          sl = sl + 1u == slots ? 0u : sl + 1u;
        }
      }
      while (k < n_out && m < t0 + cnt) {   // every output the step has completed: input m - i at the slot i behind m's
        uint32_t si = wslot + (uint32_t)(m - t0);
        si = si >= slots ? si - slots : si;
        const Real *tp = taps + q;
        Real acc = 0;
#pragma unroll 4
        for (uint32_t i = 0; i < k_full; i++) {
          acc = mac(acc, tp[(size_t)i * Lu], dl[si * kPitch + lane]);
          si = si == 0u ? slots - 1u : si - 1u;
        }
        if (ph < rem) acc = mac(acc, tp[(size_t)k_full * Lu], dl[si * kPitch + lane]);
        const uint32_t code = F::encode((float)acc);
        const uint32_t kk = (uint32_t)(k & (size_t)(kTile - 1));
        reinterpret_cast<Bits *>(codes + lane * kRowPitch)[kk] = (Bits)code;
        if (kk == (uint32_t)kTile - 1u || k + 1 == n_out) {
          __syncthreads();
          store_code_rows(codes, out, out_pitch, k - kk, n_out, M.n_streams, vec_ok, lane);
          __syncthreads();   // (the rows' readers, before the next tile's codes)
        }
        k++;
        q = q + 1u == Lu ? 0u : q + 1u;
        ph += Md;
        while (ph >= Lu) { ph -= Lu; m++; }
      }
      wslot = sl;
    }
    // the history after the call: samples n_high - H + h, at slot (n_high + h) mod slots
    __syncthreads();
    const uint32_t hbase = (uint32_t)(n_high % slots);
    for (uint32_t c = 0; c < 64u; c++) {
      const uint32_t s = blockIdx.x * 64u + c;
      if (s >= M.n_streams) break;
      for (uint32_t h = lane; h < H; h += 64u) {
        uint32_t si = hbase + h;
        si = si >= slots ? si - slots : si;
        hist_out[(size_t)s * H + h] = dl[si * kPitch + c];
      }
    }
    if (active) {
      if (G.pos >= flen) {  // isComplete: ChunkedModulator.reset() + pendingModulation = null
        T.tx_pos[stream] = 0u; T.tx_len[stream] = 0u; T.tx_pending[stream] = 0u;
        T.tx_completed[stream] += 1u;
        if (clear_rx_on_complete) { w = 0u; r = 0u; len = 0u; rx_dirty = true; }
      } else {
        T.tx_phase[stream] = G.phase; T.tx_pos[stream] = G.pos; T.tx_in_bit[stream] = G.in_bit;
        T.tx_bit_idx[stream] = G.bit_idx; T.tx_cur_bit[stream] = G.cur_bit;
      }
    }
  }
  if (rx_dirty && valid) { T.rx_w[stream] = w; T.rx_r[stream] = r; T.rx_len[stream] = len; }
}

// startModulation() for the selected streams: take the payload, arm the generator at sample 0
__global__ void processor_tx_start_kernel(ModParams M, ProcState T, const uint8_t *__restrict__ payloads,
                                          const uint32_t *__restrict__ lens, size_t payload_pitch,
                                          const uint8_t *__restrict__ mask) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= M.n_streams) return;
  if (mask && !mask[s]) return;
  const uint32_t n = lens[s];
  T.tx_pending[s] = 1u;
  T.tx_pos[s] = 0u;
  if (n == 0u) {  // startModulation(empty) -> reset(): no signal, the modulator object stays pending
    T.tx_len[s] = 0u;
    T.tx_n_payload[s] = 0u;
    return;
  }
  for (uint32_t i = 0; i < n; i++) T.tx_payload[(size_t)s * T.tx_payload_pitch + i] = payloads[(size_t)s * payload_pitch + i];
  FrameGen G;
  G.start(M, 0.0, 0.0, n);
  T.tx_n_payload[s] = n;
  T.tx_len[s] = G.frame_len;
  T.tx_phase[s] = 0.0;
  T.tx_in_bit[s] = G.in_bit; T.tx_bit_idx[s] = G.bit_idx; T.tx_cur_bit[s] = G.cur_bit;
}

// demodulate(): remove everything buffered, oldest first
__global__ void processor_rx_drain_kernel(ProcState T, uint32_t n_streams, uint8_t *__restrict__ out, size_t out_pitch,
                                          uint32_t *__restrict__ counts) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  uint32_t r = T.rx_r[s];
  const uint32_t len = T.rx_len[s];
  const uint8_t *ring = T.rx_buf + (size_t)s * T.rx_cap;
  for (uint32_t i = 0; i < len; i++) {
    if ((size_t)i < out_pitch) out[(size_t)s * out_pitch + i] = ring[r];
    r = r + 1 == T.rx_cap ? 0u : r + 1;
  }
  counts[s] = len;
  T.rx_r[s] = r;
  T.rx_len[s] = 0u;
}

// FSKProcessor.reset() (fsk-processor.ts:140-146) / ChunkedModulator.cancel(); stream < 0 = all
__global__ void processor_reset_kernel(ProcState T, uint32_t n_streams, int64_t stream, int rx, int tx) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  if (stream >= 0 && (int64_t)s != stream) return;
  if (rx) { T.rx_w[s] = 0u; T.rx_r[s] = 0u; T.rx_len[s] = 0u; }
  if (tx) { T.tx_pending[s] = 0u; T.tx_len[s] = 0u; T.tx_pos[s] = 0u; }
}

hipError_t launch_processor_io(const ModParams &M, const double *coef, const ProcState &T, const uint8_t *demod_out,
                               size_t demod_pitch, const uint32_t *demod_counts, bool do_rx, float *out, size_t n_out,
                               size_t out_pitch, bool clear_rx_on_complete, hipStream_t st) {
  const uint32_t blocks = (M.n_streams + 63u) / 64u;
  const int vec_ok = out && (out_pitch % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15u) == 0);
  if (M.exact_sin)
    hipLaunchKernelGGL(processor_io_kernel<true>, dim3(blocks), dim3(64), 0, st, M, coef, T, demod_out, demod_pitch,
                       demod_counts, do_rx ? 1 : 0, out, n_out, out_pitch, vec_ok, clear_rx_on_complete ? 1u : 0u);
  else
    hipLaunchKernelGGL(processor_io_kernel<false>, dim3(blocks), dim3(64), 0, st, M, coef, T, demod_out, demod_pitch,
                       demod_counts, do_rx ? 1 : 0, out, n_out, out_pitch, vec_ok, clear_rx_on_complete ? 1u : 0u);
  return hipGetLastError();
}
// every format-writing instantiation, once: [exact sine][format][layout] in the order of include/fskhip.h's enums; float32
// stream-major is processor_io_kernel's
#define FSK_IO_FMT_ROW(EXACT, FMT) {FSK_K(processor_io_fmt_kernel, EXACT, FMT, FSKHIP_LAYOUT_STREAM_MAJOR), FSK_K(processor_io_fmt_kernel, EXACT, FMT, FSKHIP_LAYOUT_SAMPLE_MAJOR)}
#define FSK_IO_FMT_KERNELS(EXACT)                                                                                                   \
  {{{nullptr, nullptr}, FSK_K(processor_io_fmt_kernel, EXACT, FSKHIP_SAMPLES_F32, FSKHIP_LAYOUT_SAMPLE_MAJOR)}, FSK_IO_FMT_ROW(EXACT, FSKHIP_SAMPLES_S16), \
   FSK_IO_FMT_ROW(EXACT, FSKHIP_SAMPLES_MULAW), FSK_IO_FMT_ROW(EXACT, FSKHIP_SAMPLES_ALAW)}
using IoFmtFn = void (*)(ModParams, const double *, ProcState, const uint8_t *, size_t, const uint32_t *, int, void *, size_t, size_t, int, uint32_t);
static const KernelEntry<IoFmtFn> kIoFmtKernels[2][4][2] = {FSK_IO_FMT_KERNELS(false), FSK_IO_FMT_KERNELS(true)};

hipError_t launch_processor_io_fmt(const ModParams &M, const double *coef, const ProcState &T, const uint8_t *demod_out,
                                   size_t demod_pitch, const uint32_t *demod_counts, bool do_rx, void *out, int format, int layout,
                                   size_t n_out, size_t out_pitch, bool clear_rx_on_complete, hipStream_t st) {
  if (format == FSKHIP_SAMPLES_F32 && layout == FSKHIP_LAYOUT_STREAM_MAJOR)
    return launch_processor_io(M, coef, T, demod_out, demod_pitch, demod_counts, do_rx, (float *)out, n_out, out_pitch, clear_rx_on_complete, st);
  const uint32_t blocks = (M.n_streams + 63u) / 64u;
  const size_t esz = sample_bytes(format);
  const int vec_ok = out && (out_pitch * esz % 16 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15u) == 0);
  hipLaunchKernelGGL(kIoFmtKernels[M.exact_sin ? 1 : 0][format][layout].fn, dim3(blocks), dim3(64), 0, st, M, coef, T, demod_out, demod_pitch,
                     demod_counts, do_rx ? 1 : 0, out, n_out, out_pitch, vec_ok, clear_rx_on_complete ? 1u : 0u);
  return hipGetLastError();
}
// every low rate instantiation, once: [exact sine][the decimator's precision][format] in the order of the headers' enums
#define FSK_IO_RATE_KERNELS(EXACT, R) \
  {FSK_K(processor_io_rate_kernel, EXACT, R, FSKHIP_SAMPLES_F32), FSK_K(processor_io_rate_kernel, EXACT, R, FSKHIP_SAMPLES_S16), \
   FSK_K(processor_io_rate_kernel, EXACT, R, FSKHIP_SAMPLES_MULAW), FSK_K(processor_io_rate_kernel, EXACT, R, FSKHIP_SAMPLES_ALAW)}
using IoRateFn = void (*)(ModParams, const double *, ProcState, const uint8_t *, size_t, const uint32_t *, int, void *, size_t, size_t, int, uint32_t, const float *,
                          float *, const void *, uint32_t, uint32_t, uint32_t);
static const KernelEntry<IoRateFn> kIoRateKernels[2][2][4] = {{FSK_IO_RATE_KERNELS(false, float), FSK_IO_RATE_KERNELS(false, double)},
                                                              {FSK_IO_RATE_KERNELS(true, float), FSK_IO_RATE_KERNELS(true, double)}};

hipError_t launch_processor_io_rate(const ModParams &M, const double *coef, const ProcState &T, const uint8_t *demod_out, size_t demod_pitch,
                                    const uint32_t *demod_counts, bool do_rx, void *out, int format, int layout, size_t n_out, size_t out_pitch,
                                    bool clear_rx_on_complete, int precision, uint32_t factor, uint32_t n_taps, const void *d_taps, const float *d_hist_in,
                                    float *d_hist_out, hipStream_t st) {
  const size_t esz = sample_bytes(format);
  const RatePlan P = processor_rate_plan(factor, n_taps, (uint32_t)esz, layout == FSKHIP_LAYOUT_STREAM_MAJOR);
  if (!out || n_out == 0 || !P.fused) return hipErrorInvalidValue;
  const uint32_t blocks = (M.n_streams + 63u) / 64u;
  const int vec_ok = (out_pitch * esz % 16 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15u) == 0);
  hipLaunchKernelGGL(kIoRateKernels[M.exact_sin ? 1 : 0][precision == FSKHIP_PRECISION_F64 ? 1 : 0][format].fn, dim3(blocks), dim3(64), P.lds_bytes, st, M,
                     coef, T, demod_out, demod_pitch, demod_counts, do_rx ? 1 : 0, out, n_out, out_pitch, vec_ok, clear_rx_on_complete ? 1u : 0u, d_hist_in,
                     d_hist_out, d_taps, factor, n_taps, P.slots);
  return hipGetLastError();
}
// every instantiation behind a playback converter, once: [exact sine][the converter's precision][format], as above
// (and in front: [any length], the form of the body)
#define FSK_IO_RATECVT_KERNELS(EXACT, R, ANY) \
  {FSK_K(processor_io_ratecvt_kernel, EXACT, R, FSKHIP_SAMPLES_F32, ANY), FSK_K(processor_io_ratecvt_kernel, EXACT, R, FSKHIP_SAMPLES_S16, ANY), \
   FSK_K(processor_io_ratecvt_kernel, EXACT, R, FSKHIP_SAMPLES_MULAW, ANY), FSK_K(processor_io_ratecvt_kernel, EXACT, R, FSKHIP_SAMPLES_ALAW, ANY)}
#define FSK_IO_RATECVT_FORM(ANY) \
  {{FSK_IO_RATECVT_KERNELS(false, float, ANY), FSK_IO_RATECVT_KERNELS(false, double, ANY)}, \
   {FSK_IO_RATECVT_KERNELS(true, float, ANY), FSK_IO_RATECVT_KERNELS(true, double, ANY)}}
using IoRatecvtFn = void (*)(ModParams, const double *, ProcState, const uint8_t *, size_t, const uint32_t *, int, void *, size_t, size_t, int, uint32_t, const float *,
                             float *, const void *, uint32_t, uint32_t, uint32_t, uint32_t, size_t, uint32_t, uint32_t, uint32_t);
static const KernelEntry<IoRatecvtFn> kIoRatecvtKernels[2][2][2][4] = {FSK_IO_RATECVT_FORM(false), FSK_IO_RATECVT_FORM(true)};

hipError_t launch_processor_io_ratecvt(const ModParams &M, const double *coef, const ProcState &T, const uint8_t *demod_out, size_t demod_pitch,
                                       const uint32_t *demod_counts, bool do_rx, void *out, int format, int layout, size_t n_out, size_t out_pitch,
                                       bool clear_rx_on_complete, int precision, uint32_t up, uint32_t down, uint32_t pos, size_t n_high,
                                       uint32_t n_taps, const void *d_taps, const float *d_hist_in, float *d_hist_out, hipStream_t st) {
  const size_t esz = sample_bytes(format);
  const RatePlan P = processor_ratecvt_plan(up, n_taps, (uint32_t)esz, layout == FSKHIP_LAYOUT_STREAM_MAJOR);
  if (!out || n_out == 0 || pos >= down || !P.fused) return hipErrorInvalidValue;
  const bool any = processor_ratecvt_any(up, down, pos, n_out, n_high);
  const RatecvtStart B = processor_ratecvt_start(up, down, pos, n_out);
  if (n_high < B.n_high || ratecvt_out_count_any(up, down, pos, n_high) != n_out) return hipErrorInvalidValue;   // (samples that do not write n_out)
  const uint32_t blocks = (M.n_streams + 63u) / 64u;
  const int vec_ok = (out_pitch * esz % 16 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15u) == 0);
  hipLaunchKernelGGL(kIoRatecvtKernels[any][M.exact_sin ? 1 : 0][precision == FSKHIP_PRECISION_F64 ? 1 : 0][format].fn, dim3(blocks), dim3(64), P.lds_bytes, st,
                     M, coef, T, demod_out, demod_pitch, demod_counts, do_rx ? 1 : 0, out, n_out, out_pitch, vec_ok, clear_rx_on_complete ? 1u : 0u, d_hist_in,
                     d_hist_out, d_taps, up, down, n_taps, P.slots, n_high, B.q, B.ph, B.m);
  return hipGetLastError();
}
hipError_t launch_processor_tx_start(const ModParams &M, const ProcState &T, const uint8_t *payloads, const uint32_t *lens,
                                     size_t payload_pitch, const uint8_t *mask, hipStream_t st) {
  hipLaunchKernelGGL(processor_tx_start_kernel, dim3((M.n_streams + 255u) / 256u), dim3(256), 0, st, M, T, payloads, lens,
                     payload_pitch, mask);
  return hipGetLastError();
}
hipError_t launch_processor_rx_drain(const ProcState &T, uint32_t n_streams, uint8_t *out, size_t out_pitch,
                                     uint32_t *counts, hipStream_t st) {
  hipLaunchKernelGGL(processor_rx_drain_kernel, dim3((n_streams + 255u) / 256u), dim3(256), 0, st, T, n_streams, out,
                     out_pitch, counts);
  return hipGetLastError();
}
hipError_t launch_processor_reset(const ProcState &T, uint32_t n_streams, int64_t stream, bool rx, bool tx, hipStream_t st) {
  hipLaunchKernelGGL(processor_reset_kernel, dim3((n_streams + 255u) / 256u), dim3(256), 0, st, T, n_streams, stream,
                     rx ? 1 : 0, tx ? 1 : 0);
  return hipGetLastError();
}

// ---- AWGN ------------------------------------------------------------------------------------
// pass 1: one wave per stream, coalesced row sweep, f64 sum of squares -> sigma[s]
__global__ __launch_bounds__(64) void power_kernel(const float *__restrict__ buf, size_t n, size_t pitch,
                                                   uint32_t n_streams, double snr_db, double *__restrict__ sigma) {
  const uint32_t s = blockIdx.x;
  if (s >= n_streams) return;
  const float *row = buf + (size_t)s * pitch;
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < n; i += 64) { double v = (double)row[i]; acc += v * v; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (threadIdx.x == 0) {
    double p = n ? acc / (double)n : 0.0;
    sigma[s] = sqrt(p / pow(10.0, snr_db / 10.0));
  }
}
// pass 2: elementwise, Box-Muller on a counter-based hash of (seed, stream, sample)
__global__ __launch_bounds__(256) void awgn_kernel(float *__restrict__ buf, size_t n, size_t pitch, uint32_t s_base,
                                                   uint32_t n_streams, const double *__restrict__ sigma, uint64_t seed) {
  const uint32_t s = s_base + blockIdx.y;
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (s >= n_streams || i >= n) return;
  uint64_t h = fmix64(fmix64(seed + kGolden * (1ull + s)) ^ (kGolden * (1ull + (uint64_t)i)));
  uint64_t h2 = fmix64(h + kGolden);
  double u1 = ((double)(h >> 11) + 1.0) * (1.0 / 9007199254740992.0);  // (0,1]
  double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);
  double g = sqrt(-2.0 * log(u1)) * cos(2.0 * 3.14159265358979323846 * u2);
  float *p = buf + (size_t)s * pitch + i;
  *p = (float)((double)*p + sigma[s] * g);
}

// ---- read-pattern probe (measurement tooling) --------------------------------------------------
// Streams a [n_streams][pitch] float buffer with exactly the demodulator's fast-path access pattern
// (one wave per 64 rows, 16-sample tiles, four 16-B/lane loads of 16 rows x 64 B) and does nothing
// else, so a rocprofv3 FETCH_SIZE pass over it calibrates that counter against a known byte count
// (MI355X_MICROARCH.md, HBM: "calibrate on a known byte count in your own access pattern").
__global__ __launch_bounds__(64) void probe_read_kernel(const float *__restrict__ buf, size_t n, size_t pitch,
                                                        uint32_t n_streams, float *__restrict__ sink) {
  const uint32_t lane = threadIdx.x, sub_row = lane >> 2, chunk = lane & 3;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t t0 = 0; t0 + 16 <= n; t0 += 16) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint32_t r = blockIdx.x * 64u + 16u * i + sub_row;
      r = r < n_streams ? r : n_streams - 1;
      const float4 v = *reinterpret_cast<const float4 *>(buf + (size_t)r * pitch + t0 + 4u * chunk);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  if (acc.x + acc.y + acc.z + acc.w == 12345.678f) sink[0] = acc.x;  // keeps the loads alive
}
hipError_t launch_probe_read(const float *buf, size_t n, size_t pitch, uint32_t n_streams, float *sink, hipStream_t st) {
  hipLaunchKernelGGL(probe_read_kernel, dim3((n_streams + 63u) / 64u), dim3(64), 0, st, buf, n, pitch, n_streams, sink);
  return hipGetLastError();
}

hipError_t launch_modulate(const ModParams &M, const double *coef, const uint8_t *payloads, const uint32_t *lens,
                           size_t payload_pitch, float *out, size_t out_pitch, uint32_t *out_lens, hipStream_t st) {
  const uint32_t blocks = (M.n_streams + 63u) / 64u;
  const int vec_ok = (out_pitch % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15u) == 0);
  if (M.spb >= (uint32_t)kTile) {      // (at most one bit boundary per 32-sample tile: the uniform-control kernel)
    if (M.exact_sin)
      hipLaunchKernelGGL(modulate_wide_kernel<true>, dim3(blocks), dim3(64 * kModWaves), 0, st, M, coef, payloads, lens, payload_pitch, out,
                         out_pitch, vec_ok, out_lens);
    else
      hipLaunchKernelGGL(modulate_wide_kernel<false>, dim3(blocks), dim3(64 * kModWaves), 0, st, M, coef, payloads, lens, payload_pitch, out,
                         out_pitch, vec_ok, out_lens);
    return hipGetLastError();
  }
  if (M.exact_sin)
    hipLaunchKernelGGL(modulate_kernel<true>, dim3(blocks), dim3(64), 0, st, M, coef, payloads, lens, payload_pitch, out,
                       out_pitch, vec_ok, out_lens);
  else
    hipLaunchKernelGGL(modulate_kernel<false>, dim3(blocks), dim3(64), 0, st, M, coef, payloads, lens, payload_pitch, out,
                       out_pitch, vec_ok, out_lens);
  return hipGetLastError();
}
hipError_t launch_synth(const ModParams &M, const double *coef, float *out, size_t n, size_t pitch,
                        uint32_t payload_len, uint64_t seed, uint32_t lead_max, double amp_lo, double amp_hi,
                        hipStream_t st) {
  const uint32_t blocks = (M.n_streams + 63u) / 64u;
  const int vec_ok = (pitch % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15u) == 0);
  hipLaunchKernelGGL(synth_kernel, dim3(blocks), dim3(64), 0, st, M, coef, out, n, pitch, vec_ok, payload_len, seed,
                     lead_max, amp_lo, amp_hi);
  return hipGetLastError();
}
hipError_t launch_awgn(float *buf, size_t n, size_t pitch, uint32_t n_streams, double snr_db, uint64_t seed,
                       double *sigma, hipStream_t st) {
  hipLaunchKernelGGL(power_kernel, dim3(n_streams), dim3(64), 0, st, buf, n, pitch, n_streams, snr_db, sigma);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // grid.y is limited to 65535: sweep streams in slabs
  for (uint32_t s0 = 0; s0 < n_streams; s0 += 32768u) {
    uint32_t cnt = n_streams - s0 < 32768u ? n_streams - s0 : 32768u;
    dim3 g((unsigned)((n + 255) / 256), cnt);
    hipLaunchKernelGGL(awgn_kernel, g, dim3(256), 0, st, buf, n, pitch, s0, n_streams, sigma, seed);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

uint8_t host_synth_payload_byte(uint64_t seed, uint32_t stream, uint32_t frame, uint32_t i) {
  return synth_payload_byte(seed, stream, frame, i);
}
void host_synth_stream_params(uint64_t seed, uint32_t stream, uint32_t lead_max, double amp_lo, double amp_hi,
                              uint32_t *lead, double *amp) {
  synth_stream_params(seed, stream, lead_max, amp_lo, amp_hi, lead, amp);
}

}  // namespace fsk
