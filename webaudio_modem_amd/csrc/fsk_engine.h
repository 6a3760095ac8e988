// fsk_engine.h -- struct fskhip_engine and the engine functions more than one C-ABI unit calls (not part of the ABI).
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fsk_host.h"
#include "fsk_params.h"
#include "fsk_plan.h"

struct fskhip_engine {
  int device = 0;
  int precision = 0;
  uint32_t n_streams = 0;
  fskhip_config cfg0{};
  std::vector<fskhip_config> cfgs;   // as given to fskhip_create: one (shared) or one per stream
  uint32_t matched_zero = 0;         // `matched` of a stream with an all-zero bit history (init_kernel)
  fsk::DemodParams P{};
  fsk::ModParams M{};
  fsk::DemodState S{};
  size_t lds_bytes = 0;
  uint32_t n_blocks = 0;
  int cus = 0;                       // compute units of the device (0: the query failed)
  // modulator geometry (doubles as in the reference)
  double spb = 0, bpb = 0;
  // host-side debug counters (fsk.ts:131): engine-wide totals minus per-stream baselines
  uint64_t calls = 0, total_samples = 0;
  std::vector<uint64_t> base_calls, base_samples;
  bool ds_uniform = true;
  uint32_t ds_parity = 0;        // downsample.counter shared by all streams while ds_uniform
  uint64_t pushes = 0;           // decimated samples since create (lock-step engines): the amplitude ring's write position
  bool gen_odd = false;          // fp32: the last generic-kernel launch left a decimator pair open (its partial sums are in
                                 // the reference's frame, the whole-tile kernels' in the free-running one)
  bool demodulated = false;      // a demodulate call has been issued or replayed (fskhip_set_option refuses from then on)
  const char *last_kernel = "";  // what the last fskhip_demodulate_device call launched for its whole tiles, as the launcher named it (fsk_launch.h)
  uint32_t handoff_fault = 0;    // sticky: a kernel's hand-off wait ran into its bound (csrc/fsk_wait.h)
  bool demod_ok = true;          // false: configuration the demodulator kernels do not implement
  std::string demod_why;
  uint32_t trace_cap = 0;
  // what fskhip_set_option() can change (tests and measurements; none changes a result)
  bool force_generic = false;    // "force_generic": never a whole-tile kernel
  fsk::KernelPolicy policy = fsk::KernelPolicy::AUTO;   // "kernel": which whole-tile kernels fp32 lock-step calls may use (fsk_plan.h)
  uint32_t split_cus = 256;      // compute units the two-wave kernel's residency rule counts with (cus, or 256 where unknown)
  // the exact path (fp64, fsk_demod.hip) on two waves per 64-stream group -- loads + AGC + pre-filter | the rest (SPLIT2): 0 never
  // (the default: measured SLOWER, 156 against 180 Gsamples/s at config #3 -- at two waves per SIMD the back wave has 256 registers and
  // spills 864 bytes per lane, where the one-wave kernel spreads into the accumulation registers), 1 wherever it applies
  // ("exact_waves" = 2: bit-identical, tests/test_gpu_parity.py), 2 batches of at most one group per SIMD
  uint32_t exact_split = 0;
  size_t host_slab = (size_t)-1; // samples per time slab of fskhip_demodulate_host's pipeline ((size_t)-1 = ~96 MB, 0 = no pipeline)
  struct Blk {                   // the four-wave kernel's tuning state
    uint32_t resident = 0;       // workgroups of demod_blk_kernel the device holds at once; larger batches run it persistent, in time slices
    uint32_t min_tiles = 0;      // calls with fewer whole tiles than this stay with round 2's kernels
    uint32_t y_slots = 6;        // half tiles in the block kernel's y ring: as deep as the LDS allows at this batch size
    bool y_pinned = false;       // "blk_y_slots" was set: "blk_lanes" leaves it alone
    uint32_t lanes = 64;         // streams per workgroup of demod_blk_kernel: 64, or 32 / 16 / 8 for batches that leave CUs idle (fsk_blk.hip)
    uint32_t slice_tiles = 0;    // tiles per time slice (0 = the kernel file's default, 0xFFFFFFFF = never slice)
    // "blk_resets": which of fsk_blk.hip's two kernels a call launches -- demod_blk_kernel_r, whose block path takes 'eod' resets
    // itself, pays where resets are frequent (an idle receiver bank: +50 %) and costs ~4 % where they are rare.  auto: by the
    // share of tiles the PREVIOUS call's back waves took off their fast loop (the kernels count; the totals come back with an
    // asynchronous 8-byte copy behind every launch and are looked at, without waiting, before the next one).
    uint32_t medium = 3;         // 0 never, 1 always, 2 (tests) always + redo every such block sample by sample, 3 auto
    bool med_now = false;        // auto's current choice
    volatile unsigned long long *h_stat = nullptr;   // pinned: {tiles, tiles off the fast loop}, {hand-off fault word, -} as the last completed copy left them
    uint32_t stat_tiles = 0, stat_rare = 0;          // ... as of the last look
    uint32_t stat_skip = 0;                          // short calls since the last fetch
  } blk;
  // seven waves per group (demod_blk6_kernel, fsk_blk6.hip): the whole-tile kernel of batches small enough to give every workgroup a
  // compute unit of its own (uniform configurations, calls of at least min_tiles tiles)
  struct Six {
    uint32_t min_tiles = 8;      // shorter calls stay on the four-wave kernel (one 128-sample quantum is already 1.13 x faster on seven waves, profiles/r05_lag.txt)
    uint32_t y_slots = 0;        // 0 = as deep as the LDS allows
    uint32_t rolemap = 0;        // 0 = the default placement of the seven parts on a workgroup's waves
  } six;
  struct Host {                  // scratch for the _host entry points
    hipStream_t stream = nullptr;
    float *d_samples = nullptr; size_t d_samples_cap = 0;
    float *d_samples2 = nullptr; size_t d_samples2_cap = 0;   // second time slab of fskhip_demodulate_host's pipeline
    hipStream_t copy_stream = nullptr;                        // its H2D stream
    uint8_t *d_narrow[2] = {nullptr, nullptr}; size_t d_narrow_cap[2] = {0, 0};   // fskhip_demodulate_host_fmt: the samples as they crossed PCIe, per time slab
    uint8_t *d_egress = nullptr; size_t d_egress_cap = 0;     // fskhip_modulate_host_fmt: the samples as they cross PCIe
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_used_up[2] = {nullptr, nullptr};
    uint8_t *d_out = nullptr; size_t d_out_cap = 0;
    uint32_t *d_counts = nullptr, *d_eod = nullptr, *d_lens = nullptr;
    uint8_t *d_payloads = nullptr; size_t d_payloads_cap = 0;
  } host;
  void *d_status = nullptr;                // fskhip_get_status: one StatusRaw (fsk_state.hip)
  double *d_sigma = nullptr;
  unsigned long long *d_clock = nullptr;   // fskhip_clock_probe_*: {shader cycles, 100 MHz ticks}
  struct Timing {                          // fskhip_timing_begin / _end: an event pair around every bracketed call
    bool on = false;
    std::vector<hipEvent_t> ev; size_t used = 0;   // created as needed; in use since fskhip_timing_begin
    hipStream_t stream = nullptr;
  } timing;
};

namespace fsk {
static constexpr size_t kStatusRawBytes = 2 * sizeof(double) + 6 * sizeof(uint32_t);
inline size_t engine_real_bytes(const fskhip_engine *e) { return e->precision == FSKHIP_PRECISION_F64 ? sizeof(double) : sizeof(float); }
// byte offset of row `f` of the real-valued state (fsk_params.h: [field][stream])
inline size_t engine_real_row(const fskhip_engine *e, int f) { return (size_t)f * e->n_streams * engine_real_bytes(e); }
// upper bound on the bytes one call can return per stream: a byte takes bitsPerByte (>= 8) bit times of spb samples
inline size_t engine_max_bytes(const fskhip_engine *e, size_t n_per_stream) { return n_per_stream / (4 * (size_t)(e->M.spb ? e->M.spb : 1)) + 8; }
// fsk_dispatch.hip
uint32_t engine_launch_key(const fskhip_engine *e);          // changes whenever the demodulator would launch differently
void engine_refresh_kernel_choice(fskhip_engine *e);         // "blk_resets" = auto: look at the tile statistics the last completed call left
void engine_note_replayed_call(fskhip_engine *e, size_t n);  // host-side counters of a call replayed from a graph
int handoff_check(fskhip_engine *e, bool blocking);
// fsk_create.hip: what a destination engine continues streams FROM -- a live engine (fskhip_remap_streams) or a snapshot of one
// (fskhip_restore_streams, fsk_snapshot_api.hip) -- and the checks, lock-step decision and host-side counters the two share
struct StreamSource {
  const char *who;                  // the entry point, for messages
  const char *the, *unit, *item;    // "the source" / "streams" / "source stream"
  int precision;
  uint32_t n_streams;
  fskhip_config cfg0;
  uint32_t d, amp_cap, wide, frac, n_bits, ring_cap;   // the geometry both sides must share
  uint64_t calls, total_samples, pushes;
  uint32_t ds_parity, quality;
  bool ds_uniform, gen_odd;
  const void *ctx;
  fskhip_config (*config)(const void *ctx, size_t s);
  void (*baselines)(const void *ctx, size_t s, uint64_t *calls, uint64_t *samples);
};
struct RemapPlan {
  uint32_t n_fresh;      // map entries of -1
  int64_t frame_row;     // the first continued stream's source row, or -1
  bool uniform, gen_odd; // what the destination's ds_uniform / gen_odd become
  uint32_t parity;
  bool grid;             // new streams take the source's ring positions
  bool frame;            // new streams join the free-running I/Q frame of source row frame_row
};
int remap_check_map(const char *who, const char *what, const int64_t *map, uint32_t n_map);
int remap_check(const fskhip_engine *dst, const StreamSource &V, const int64_t *map, uint32_t n_map, RemapPlan *plan);
void remap_finish(fskhip_engine *dst, const StreamSource &V, const int64_t *map, uint32_t n_map, const RemapPlan &plan);
int engine_refuse_handoff(const char *who, const char *the, const fskhip_engine *e);
bool config_shared_fields_equal(const fskhip_config &a, const fskhip_config &b);
bool config_all_fields_equal(const fskhip_config &a, const fskhip_config &b);   // what a continued stream and its source must share
const fskhip_config &engine_stream_config(const fskhip_engine *e, size_t s);
// fsk_api.hip: the event pair fskhip_timing_begin / _end put around a call's launches (nothing while timing is off)
int timing_open(fskhip_engine *e, hipStream_t st);
int timing_close(fskhip_engine *e, hipStream_t st);
}  // namespace fsk
