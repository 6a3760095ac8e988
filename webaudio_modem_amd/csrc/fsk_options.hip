// fsk_options.hip -- fskhip_set_option and the engine's read-only getters (include/fskhip.h).
#include <cstdlib>

#include "fsk_engine.h"
#include "fsk_launch.h"

using namespace fsk;

extern "C" {
// Tuning and test switches (include/fskhip.h).  Everything here only chooses among kernels / launch shapes that compute the
// same bytes; the library itself reads no environment variable (the switches used to be
// unvalidated getenv() calls inside fskhip_create).
int fskhip_set_option(fskhip_engine *e, const char *name, const char *value) {
  if (!e || !name || !value) return fail(FSKHIP_E_INVALID, "fskhip_set_option: null argument");
  // (a flag of this engine's own calls -- not the call counters, which fskhip_carry_over copies from the old engine: ADVICE r04)
  if (e->demodulated) return fail(FSKHIP_E_INVALID, "fskhip_set_option(%s): the engine has demodulated already (set options after fskhip_create / fskhip_carry_over, before the first demodulate call)", name);
  const std::string k(name), v(value);
  auto number = [&](uint64_t lo, uint64_t hi, auto *out) -> int {   // a decimal number in [lo, hi] into *out, whatever its type
    if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 12)
      return fail(FSKHIP_E_INVALID, "fskhip_set_option(%s): '%s' is not a number", name, value);
    const uint64_t x = strtoull(v.c_str(), nullptr, 10);
    if (x < lo || x > hi) return fail(FSKHIP_E_INVALID, "fskhip_set_option(%s): %s outside [%llu, %llu]", name, value, (unsigned long long)lo, (unsigned long long)hi);
    *out = static_cast<std::remove_pointer_t<decltype(out)>>(x);
    return FSKHIP_OK;
  };
  uint64_t x = 0; int rc;
  if (k == "kernel") {          // which whole-tile kernel fp32 lock-step calls use ("six-wave": the seven-wave kernel's first name)
    static const struct { const char *name; KernelPolicy policy; } kPolicies[] = {
        {"auto", KernelPolicy::AUTO},           {"auto-r04", KernelPolicy::AUTO_R04},    {"auto-r02", KernelPolicy::AUTO_R02}, {"seven-wave", KernelPolicy::SEVEN_WAVE},
        {"six-wave", KernelPolicy::SEVEN_WAVE}, {"four-wave", KernelPolicy::FOUR_WAVE}, {"two-wave", KernelPolicy::TWO_WAVE}, {"one-wave", KernelPolicy::ONE_WAVE}};
    for (const auto &p : kPolicies)
      if (v == p.name) { e->policy = p.policy; return FSKHIP_OK; }
    return fail(FSKHIP_E_INVALID, "fskhip_set_option(kernel): '%s' is none of auto, auto-r04, auto-r02, seven-wave, four-wave, two-wave, one-wave", value);
  }
  if (k == "blk_resets") {      // 1: the four-wave kernel's block path takes resets (default), 0: such blocks go sample by sample
    if (v == "auto") { e->blk.medium = 3u; return FSKHIP_OK; }
    return number(0, 2, &e->blk.medium);   // (2, tests: run it, then restore the entry state and redo the block sample by sample)
  }
  if (k == "stage_min_tiles") return number(0, 1u << 30, &e->six.min_tiles);
  if (k == "stage_y_slots") {     // (checked against what the kernel can use, as blk_y_slots is -- it used to be clamped silently)
    if (!(e->demod_ok && e->precision == FSKHIP_PRECISION_F32 && demod_blk6_applicable(e->P))) return FSKHIP_OK;   // (the seven-wave kernel does not apply: nothing to tune)
    const uint32_t lo = demod_blk6_min_y_slots(), hi = demod_blk6_y_slots(e->P);
    if ((rc = number(lo, hi, &x)) != FSKHIP_OK) return rc;
    if (x & 1u) return fail(FSKHIP_E_INVALID, "fskhip_set_option(stage_y_slots): %s is odd (whole tiles: two half tiles each)", value);
    e->six.y_slots = (uint32_t)x;
    return FSKHIP_OK;
  }
  if (k == "stage_roles") {       // measurements: the part each of the seven waves plays, e.g. 0135426 (every part exactly once)
    if (v == "auto") { e->six.rolemap = 0u; return FSKHIP_OK; }
    uint32_t m = 0, seen = 0;
    if (v.size() != 7) return fail(FSKHIP_E_INVALID, "fskhip_set_option(stage_roles): '%s' is not seven digits 0..6", value);
    for (uint32_t w = 0; w < 7; w++) {
      const uint32_t r = (uint32_t)(v[w] - '0');
      if (r > 6u || (seen & (1u << r))) return fail(FSKHIP_E_INVALID, "fskhip_set_option(stage_roles): '%s' is not a permutation of 0..6", value);
      seen |= 1u << r; m |= r << (3u * w);
    }
    e->six.rolemap = m;
    return FSKHIP_OK;
  }
  if (k == "exact_waves") {       // the fp64 kernel: auto | 1 (one wave per 64-stream group) | 2 (two: loads + AGC + pre-filter | the rest)
    if (v == "auto") { e->exact_split = 0u; return FSKHIP_OK; }     // (auto = one wave: the two-wave cut does not pay, see exact_split)
    if ((rc = number(1, 2, &x)) != FSKHIP_OK) return rc;
    e->exact_split = x == 2 ? 1u : 0u;
    return FSKHIP_OK;
  }
  if (k == "force_generic") return number(0, 1, &e->force_generic);
  if (k == "host_slab") return number(0, 1ull << 40, &e->host_slab);
  const bool blk = e->demod_ok && e->precision == FSKHIP_PRECISION_F32 && demod_blk_applicable(e->P);
  if (k == "blk_y_slots" || k == "blk_min_tiles" || k == "blk_resident" || k == "slice_tiles" || k == "blk_lanes") {
    if (!blk) return FSKHIP_OK;                       // (the four-wave kernel does not apply to this engine: nothing to tune)
    if (k == "blk_y_slots") {
      if ((rc = number(6, 28, &x)) != FSKHIP_OK) return rc;
      if (demod_blk_lds_bytes(e->P, (uint32_t)x) > kLdsLimit)
        return fail(FSKHIP_E_INVALID, "fskhip_set_option(blk_y_slots): %s slots need %zu B of LDS (> 160 KiB) at dsSPB %u", value,
                    demod_blk_lds_bytes(e->P, (uint32_t)x), e->P.d);
      e->blk.y_slots = (uint32_t)x;
      e->blk.y_pinned = true;                          // (a later "blk_lanes" re-plans the depth only if it was not asked for)
    } else if (k == "blk_lanes") {                    // streams per workgroup: auto (what the device's CU count suggests) | 64 | 32 | 16 | 8
      if (v != "auto") {
        if ((rc = number(8, 64, &x)) != FSKHIP_OK) return rc;
        if (x & (x - 1u)) return fail(FSKHIP_E_INVALID, "fskhip_set_option(blk_lanes): %s is none of auto, 64, 32, 16, 8", value);
      }
      e->blk.lanes = v == "auto" ? demod_blk_lanes(e->n_streams, e->device) : (uint32_t)x;
      // the ring depth follows the workgroup count the new width gives; a "blk_resident" pinned by a test stays
      uint32_t y = 0, res = 0;
      demod_blk_plan(e->P, (e->n_streams + e->blk.lanes - 1u) / e->blk.lanes, e->device, &y, &res);
      if (y && !e->blk.y_pinned) e->blk.y_slots = y;
    } else if (k == "blk_min_tiles") {
      return number(0, 1u << 30, &e->blk.min_tiles);
    } else if (k == "blk_resident") {                 // tests: a "device" that holds only this many workgroups at once
      if ((rc = number(1, 1u << 20, &x)) != FSKHIP_OK) return rc;
      e->blk.resident = (uint32_t)x;
      e->blk.lanes = 64u;                             // (a device that small has no idle CUs to spread narrow groups over)
      if (e->n_blocks > e->blk.resident && !e->S.blk_q) {
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipMalloc((void **)&e->S.blk_q, sizeof(uint32_t) * demod_blk_queue_words(e->n_blocks)));
      }
    } else {
      if (v == "off") { e->blk.slice_tiles = 0xFFFFFFFFu; return FSKHIP_OK; }
      return number(1, 1u << 24, &e->blk.slice_tiles);
    }
    return FSKHIP_OK;
  }
  return fail(FSKHIP_E_INVALID, "fskhip_set_option: unknown option '%s'", name);
}
uint32_t fskhip_n_streams(const fskhip_engine *e) { return e ? e->n_streams : 0; }
size_t fskhip_max_bytes(const fskhip_engine *e, size_t n_per_stream) { return e ? engine_max_bytes(e, n_per_stream) : 0; }
const char *fskhip_last_kernel(const fskhip_engine *e) { return e ? e->last_kernel : ""; }
uint32_t fskhip_blk_lanes(const fskhip_engine *e) {
  return (e && e->demod_ok && e->precision == FSKHIP_PRECISION_F32 && demod_blk_applicable(e->P)) ? e->blk.lanes : 0u;
}
int fskhip_demod_supported(const fskhip_engine *e) { return e && e->demod_ok ? 1 : 0; }
}  // extern "C"
