// fsk_plan.h -- which kernels a demodulate call runs on: plain integer arithmetic over a POD of facts, no device code and no
// engine, so that the CPU suite can compile and test every rule by itself (tests/test_plan_cpu.py).  fsk_dispatch.hip fills the
// facts from the engine (plan_facts) and issues what plan_launches chose.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fsk_blk_sched.h"

namespace fsk {

static constexpr size_t kLdsLimit = 160 * 1024;   // LDS of one compute unit

// fskhip_set_option("kernel", ...), one value per spelling.  AUTO_R04: round 4's choice (never seven waves); AUTO_R02: round 2's
// (never four either).  A pinned kernel skips the residency and minimum-length checks of every family; where it does not apply at
// all the call runs on the next one down (seven -> four -> two -> one wave).
enum class KernelPolicy : uint32_t { AUTO, AUTO_R04, AUTO_R02, SEVEN_WAVE, FOUR_WAVE, TWO_WAVE, ONE_WAVE };
inline bool policy_pinned(KernelPolicy p) { return p >= KernelPolicy::SEVEN_WAVE; }
inline bool policy_four_wave(KernelPolicy p) { return p != KernelPolicy::AUTO_R02 && p < KernelPolicy::TWO_WAVE; }   // the four-wave family: seven waves too

struct PlanFacts {
  KernelPolicy policy;
  bool f64, lock_step, fast;     // fp64 engine; every stream's /2 decimator at one parity (ds_uniform); a lock-step fp32 engine with
                                 // narrow integer-capacity rings (demod_fast_applicable)
  uint32_t ds_parity, ring_pos;  // that parity; the amplitude ring's write position mod 4 (pushes & 3)
  bool gen_odd, force_generic, diagnostics;       // diagnostics: a trace or the quality estimates are on
  size_t n, pitch;               // the call's; ptr_low: the sample pointer's low two bits
  uint32_t ptr_low, n_streams, n_blocks, cus, split_cus;   // cus: 0 = unknown; split_cus: the same, 256 where unknown
  // four waves (fsk_blk.hip): demod_blk_applicable, whether the slice queue exists, the kernel's LDS bytes, the engine's blk.*
  bool blk_applicable, blk_queue;
  size_t blk_lds;
  uint32_t blk_lanes, blk_resident, blk_slice_tiles, blk_min_tiles;
  // seven waves (fsk_blk6.hip): y_pinned 0 = "stage_y_slots" not set, the call takes y_default
  bool six_applicable;
  size_t six_max_samples;
  uint32_t six_min_tiles, six_y_pinned, six_y_default;
  size_t pipe_lds, split2_lds;   // LDS bytes of the two-wave kernel (fsk_pipe.hip) and of the exact path's two-wave cut (fsk_demod.hip)
  uint32_t exact_split;          // the exact path (fp64) on two waves: 0 never, 1 wherever it applies, 2 small batches
  bool wide_or_frac;
};

enum TileKernel { K_GENERIC, K_SAMPLES, K_SEVEN_WAVE, K_FOUR_WAVE, K_TWO_WAVE, K_ONE_WAVE };
struct LaunchPlan {
  TileKernel kernel = K_GENERIC;   // K_GENERIC: all n samples on fsk_demod.hip's kernel; K_SAMPLES: all of them sample by sample (head = n)
  size_t head = 0, n_fast = 0;     // single samples in front of the whole tiles; the whole tiles' samples (the tail is what is left)
  uint32_t med = 0, y_slots = 0;   // four waves: "blk_resets" as this call takes it (the caller's, after planning); seven waves: depth of the y ring
  bool split2 = false;             // generic fp64 kernel on two waves per group
};

// The head: single samples (demod_tail_kernel) until the /2 decimator is at a pair boundary AND, for the four-wave family, the
// amplitude ring's write position is a multiple of four -- what the block kernel's quad stores need (fsk_dev.h).  At most seven
// samples.  The tile loads that follow are 16 bytes per lane from dword-aligned addresses: a buffer that is 16-byte aligned after
// the head is the common case and the fastest, but nothing depends on it (round 3 demanded both, so one odd-length
// call left an aligned device buffer on the per-sample kernel until the parity flipped back, and a call that left the ring off
// its quad grid kept the engine on round 2's kernels for good).
inline size_t plan_head(uint32_t ds_parity, uint32_t ring_pos, bool quad_grid) {
  const uint32_t at = ring_pos + ds_parity;   // the ring's position once the open pair is closed (by one sample)
  return ds_parity + (quad_grid ? 2u * (size_t)((4u - (at & 3u)) & 3u) : 0u);
}
// ... and what the host forms do about it: device copies keep a row pitch that is a multiple of 4 floats so the 16-B tile loads
// apply, and a lock-step fp32 stream whose head is odd (its decimator is mid-pair: an earlier call had an odd length) is staged
// THREE floats into its row: the one sample that closes the pair then also reaches the next 16-byte boundary -- staged at the
// row start every later even-length call would start its tiles off that boundary (fsk_api.hip's silent
// performance cliff).
inline size_t host_stage_shift(bool f64, bool lock_step, uint32_t ds_parity) {
  return (!f64 && lock_step && (plan_head(ds_parity, 0, false) & 1u)) ? 3 : 0;
}

// fskhip_modulate_host_fmt's staging (fsk_api.hip): the float rows the modulator writes, the narrow buffer fsk_samples.hip's egress kernel
// fills, and the ONE 2-D copy that brings it to the host -- of `rows` rows of `row_bytes` bytes, npitch * esz apart on the device.
// Stream-major rows start on 16-byte boundaries (the kernel's vector path from element 0); sample-major frames are packed, n_streams
// elements each, whatever frame pitch the caller's buffer has.
struct EgressStage {
  size_t fpitch;             // floats per row of the float staging: a multiple of 4
  size_t npitch;             // elements per row (stream-major) or frame (sample-major) of the narrow staging
  size_t bytes;              // of the narrow staging
  size_t rows, row_bytes;    // the copy's geometry
};
inline EgressStage egress_stage(size_t n_streams, size_t n, size_t esz, bool frames) {
  EgressStage g;
  g.fpitch = (n + 3) & ~(size_t)3;
  g.npitch = frames ? n_streams : ((n * esz + 15) & ~(size_t)15) / esz;
  g.rows = frames ? n : n_streams;
  g.row_bytes = (frames ? n_streams : n) * esz;
  g.bytes = g.rows * g.npitch * esz;
  return g;
}

// Lock-step fp32 batches with narrow integer-capacity rings never leave fsk_pipe.hip's arithmetic: a head of single samples,
// whole 16-sample tiles, a tail of single samples -- so cutting a stream into calls of any lengths changes nothing, bit for bit.
// Everything else (fp64, wide / fractional rings, streams out of lock step, an open pair the generic kernel left) is the
// generic kernel's.  Pure: the caller looks at the tile statistics and fills `med` once the four-wave family is chosen.
inline LaunchPlan plan_launches(const PlanFacts &f) {
  LaunchPlan pl;
  const bool pinned = policy_pinned(f.policy);
  if (!(f.n > 0 && !f.force_generic && !f.gen_odd && f.fast && (uint64_t)f.pitch * 4u * 64u < 0x7FFFFFF0ull)) {   // (per-wave input descriptor and offsets fit 31 bits)
    pl.split2 = f.f64 && f.lock_step && !f.wide_or_frac && !f.diagnostics && f.split2_lds <= kLdsLimit &&
                (f.exact_split == 1u || (f.exact_split == 2u && f.cus > 0 && f.n_blocks <= 4u * f.cus && f.n >= 64));
    return pl;
  }
  const bool blk = policy_four_wave(f.policy) && f.blk_applicable;
  // diagnostics (traces, quality estimates) run on the sample-granular kernel
  const bool tiles = f.pitch % 4 == 0 && f.ptr_low == 0 && !f.diagnostics;
  size_t head = plan_head(f.ds_parity, f.ring_pos, blk), n_fast = 0;
  if (tiles && head < f.n) n_fast = (f.n - head) & ~(size_t)15;
  if (!n_fast) head = f.n;   // all of it sample by sample
  pl.head = head; pl.n_fast = n_fast; pl.kernel = K_SAMPLES;
  if (!n_fast) return pl;
  // Batches beyond one round of resident workgroups run the block kernel persistently, in time slices; a call too short for two
  // slices would run it in several rounds of one workgroup per group, each paying the four-wave pipeline's fill and drain, and
  // round 2's kernels are faster there (262 144 streams x 128-sample quanta, the FSKProcessor loop: 0.195 against 0.247 ms;
  // x 4 096 samples 384 against 370 Gsamples/s: profiles/r03_short_calls.txt)
  const bool blk_fits = f.blk_lanes != 64u || !(f.blk_resident && f.n_blocks > f.blk_resident) ||
                        blk_slice_count(f.n_blocks, (uint32_t)(n_fast / 16), f.blk_resident, f.blk_slice_tiles, f.blk_queue, nullptr) >= 2u;
  if (blk && f.blk_lds <= kLdsLimit && (pinned || (blk_fits && n_fast / 16 >= f.blk_min_tiles))) {   // (behind its head the ring is on the quad grid)
    // seven waves per group: every workgroup a compute unit to itself (in narrow groups -- <= 32 streams -- the stages that are
    // not recurrences spread over the idle lanes), a call long enough to fill seven stages.  Measured against the four-wave
    // kernel: x 1.56 at 2 048 streams, x 1.48 at 4 096, x 1.42 at 8 192, x 1.13 with whole-wave groups at 16 384
    // (profiles/r05_lag.txt).  Idle receiver banks included: its frame wave takes own-span tiles on the block path with resets too.
    const uint32_t six_blocks = (f.n_streams + f.blk_lanes - 1u) / f.blk_lanes;
    const bool six = f.six_applicable && n_fast <= f.six_max_samples &&
                     (f.policy == KernelPolicy::SEVEN_WAVE ||
                      (f.policy == KernelPolicy::AUTO && f.cus > 0 && six_blocks <= f.cus && n_fast / 16 >= f.six_min_tiles));
    pl.kernel = six ? K_SEVEN_WAVE : K_FOUR_WAVE;
    if (six) pl.y_slots = f.six_y_pinned ? f.six_y_pinned : f.six_y_default;
    return pl;
  }
  // below two waves per SIMD (4 SIMDs per CU) the one-wave-per-group kernel cannot hide its own dependency stalls; the two-wave
  // kernel gives every group two instruction streams, as long as all its workgroups' LDS tiles fit on the CUs at once
  const bool want_two = pinned ? f.policy != KernelPolicy::ONE_WAVE : f.n_blocks < f.split_cus * 8u;
  const size_t wgs_per_cu = (f.n_blocks + f.split_cus - 1) / f.split_cus;
  pl.kernel = want_two && f.pipe_lds <= kLdsLimit && (pinned || wgs_per_cu * f.pipe_lds <= kLdsLimit) ? K_TWO_WAVE : K_ONE_WAVE;
  return pl;
}

}  // namespace fsk
