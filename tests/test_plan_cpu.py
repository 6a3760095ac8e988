"""Which kernels a demodulate call runs on (webaudio_modem_amd/csrc/fsk_plan.h): the planner is plain integer arithmetic over a
POD of facts, compiled here with g++ into a tiny program that plans one call per argument.  The expected values are the rules
as DESIGN.md section 4 and the header's comments state them, typed in.  CPU only."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "fsk_plan.h"
using namespace fsk;
// one call per argument, "field=value,field=value,..." over the defaults below  ->  kernel head n_fast split2 y_slots;
// "shift=1,f64=..,lock_step=..,ds_parity=.." -> host_stage_shift
int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    PlanFacts f{};
    unsigned long long policy = 0, shift = 0;
    char *row = strdup(argv[i]);
    for (char *kv = strtok(row, ","); kv; kv = strtok(nullptr, ",")) {
      char *eq = strchr(kv, '=');
      if (!eq) return 2;
      *eq = 0;
      const unsigned long long v = strtoull(eq + 1, nullptr, 10);
      bool known = false;
#define FIELD(name) if (!strcmp(kv, #name)) { f.name = (decltype(f.name))v; known = true; }
      FIELD(f64) FIELD(lock_step) FIELD(fast) FIELD(ds_parity) FIELD(ring_pos) FIELD(gen_odd) FIELD(force_generic) FIELD(diagnostics)
      FIELD(n) FIELD(pitch) FIELD(ptr_low) FIELD(n_streams) FIELD(n_blocks) FIELD(cus) FIELD(split_cus) FIELD(blk_applicable)
      FIELD(blk_queue) FIELD(blk_lds) FIELD(blk_lanes) FIELD(blk_resident) FIELD(blk_slice_tiles) FIELD(blk_min_tiles)
      FIELD(six_applicable) FIELD(six_max_samples) FIELD(six_min_tiles) FIELD(six_y_pinned) FIELD(six_y_default) FIELD(pipe_lds)
      FIELD(exact_split) FIELD(split2_lds) FIELD(wide_or_frac)
#undef FIELD
      if (!strcmp(kv, "policy")) { policy = v; known = true; }
      if (!strcmp(kv, "shift")) { shift = v; known = true; }
      if (!known) { fprintf(stderr, "unknown field %s\n", kv); return 2; }
    }
    free(row);
    f.policy = (KernelPolicy)policy;
    if (shift) { printf("%zu\n", host_stage_shift(f.f64, f.lock_step, f.ds_parity)); continue; }
    const LaunchPlan pl = plan_launches(f);
    if (pl.med != 0) return 3;   // (the caller's, after planning)
    printf("%d %zu %zu %d %u\n", (int)pl.kernel, pl.head, pl.n_fast, pl.split2 ? 1 : 0, pl.y_slots);
  }
  return 0;
}
'''

AUTO, AUTO_R04, AUTO_R02, SEVEN_WAVE, FOUR_WAVE, TWO_WAVE, ONE_WAVE = range(7)      # KernelPolicy
GENERIC, SAMPLES, SEVEN, FOUR, TWO, ONE = range(6)                                  # TileKernel
LDS = 160 * 1024
Y = 24

# a plain shape: 65 536 lock-step fp32 streams (1 024 groups of 64: exactly one round) on 256 compute units, an aligned call of
# 4 096 samples on the quad grid.  n_blocks follows n_streams unless a case says otherwise.
PLAIN = dict(policy=AUTO, f64=0, lock_step=1, fast=1, ds_parity=0, ring_pos=0, gen_odd=0, force_generic=0, diagnostics=0, n=4096,
             pitch=4096, ptr_low=0, n_streams=65536, cus=256, split_cus=256, blk_applicable=1, blk_queue=0, blk_lds=50000,
             blk_lanes=64, blk_resident=1024, blk_slice_tiles=0, blk_min_tiles=0, six_applicable=1, six_max_samples=(1 << 27) - 16,
             six_min_tiles=8, six_y_pinned=0, six_y_default=Y, pipe_lds=40000, exact_split=0, split2_lds=60000, wide_or_frac=0)
SMALL = dict(n_streams=2048, blk_lanes=8)                    # 256 narrow groups: every workgroup a compute unit to itself
F64 = dict(f64=1, fast=0)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    d = tmp_path_factory.mktemp("plan")
    (d / "t.cc").write_text(SRC)
    exe = str(d / "t")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, str(d / "t.cc")],
                   check=True)

    def run(*cases):
        """each case: dicts merged over PLAIN -> (kernel, head, n_fast, split2, y_slots)"""
        rows = []
        for case in cases:
            f = dict(PLAIN)
            for part in (case if isinstance(case, (list, tuple)) else [case]):
                f.update(part)
            f.setdefault("n_blocks", (f["n_streams"] + 63) // 64)
            rows.append(",".join("%s=%d" % kv for kv in f.items()))
        out = subprocess.run([exe] + rows, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [tuple(int(v) for v in line.split()) for line in out]
    run.exe = exe
    return run


def test_every_policy_at_a_plain_shape(plan):
    whole = lambda k, y=0: (k, 0, 4096, 0, y)
    # one round of whole-wave groups: four waves unless round 2's kernels are asked for; 1 024 groups on 256 CUs are fewer than two
    # waves per SIMD and four 40 000-byte tiles fit a CU's LDS: two waves
    assert plan(*[dict(policy=p) for p in range(7)]) == [whole(FOUR), whole(FOUR), whole(TWO), whole(SEVEN, Y), whole(FOUR), whole(TWO), whole(ONE)]
    # a batch that leaves every workgroup a compute unit: seven waves by default, "stage_y_slots" as pinned
    assert plan(*[[SMALL, dict(policy=p)] for p in range(7)]) == [whole(SEVEN, Y), whole(FOUR), whole(TWO), whole(SEVEN, Y), whole(FOUR), whole(TWO), whole(ONE)]
    assert plan([SMALL, dict(six_y_pinned=10)]) == [whole(SEVEN, 10)]


def test_head_tiles_and_tail_by_call_length(plan):
    assert plan(dict(n=0), dict(n=1), dict(n=15), dict(n=16), dict(n=17)) == [
        (GENERIC, 0, 0, 0, 0), (SAMPLES, 1, 0, 0, 0), (SAMPLES, 15, 0, 0, 0), (FOUR, 0, 16, 0, 0), (FOUR, 0, 16, 0, 0)]
    # an open pair one push short of the quad grid: the head is the one sample that closes it, the tail nothing
    assert plan(dict(n=17, ds_parity=1, ring_pos=3)) == [(FOUR, 1, 16, 0, 0)]


def test_the_head_closes_the_pair_and_reaches_the_quad_grid(plan):
    for policy in (AUTO, AUTO_R04, SEVEN_WAVE, FOUR_WAVE):
        got = plan(*[dict(policy=policy, ds_parity=p, ring_pos=r) for p in (0, 1) for r in range(4)])
        assert [g[1] for g in got] == [0, 6, 4, 2, 7, 5, 3, 1], policy
        for (p, r), g in zip([(p, r) for p in (0, 1) for r in range(4)], got):
            assert g[2] == (4096 - g[1]) // 16 * 16 and (r + (p + g[1]) // 2) % 4 == 0, (policy, p, r, g)
    # round 2's kernels store amplitudes one by one: the pair only.  So does an engine the four-wave kernel does not apply to.
    for case in (dict(policy=AUTO_R02), dict(policy=TWO_WAVE), dict(policy=ONE_WAVE), dict(blk_applicable=0)):
        got = plan(*[[case, dict(ds_parity=p, ring_pos=r)] for p in (0, 1) for r in range(4)])
        assert [g[1] for g in got] == [0, 0, 0, 0, 1, 1, 1, 1], case
    # a pinned four-wave kernel with the ring off its grid still runs four waves, behind its head
    assert plan(dict(policy=FOUR_WAVE, ring_pos=2), dict(policy=FOUR_WAVE, ring_pos=2, blk_min_tiles=1000)) == [(FOUR, 4, 4080, 0, 0)] * 2
    # a head that is the whole call, or more: sample by sample
    assert plan(dict(ds_parity=1, n=7), dict(ds_parity=1, n=5), dict(ds_parity=1, n=8), dict(ds_parity=1, n=23)) == [
        (SAMPLES, 7, 0, 0, 0), (SAMPLES, 5, 0, 0, 0), (SAMPLES, 8, 0, 0, 0), (FOUR, 7, 16, 0, 0)]


def test_what_keeps_a_call_off_whole_tiles(plan):
    per_sample, generic = (SAMPLES, 4096, 0, 0, 0), (GENERIC, 0, 0, 0, 0)
    assert plan(dict(pitch=4097), dict(pitch=4098), dict(ptr_low=1), dict(ptr_low=2), dict(diagnostics=1)) == [per_sample] * 5
    assert plan([SMALL, dict(policy=SEVEN_WAVE, diagnostics=1)]) == [per_sample]
    assert plan(dict(gen_odd=1), dict(force_generic=1), dict(fast=0), dict(policy=FOUR_WAVE, gen_odd=1)) == [generic] * 4
    # the per-wave input descriptor: 64 rows of `pitch` floats within 31 bits
    assert plan(dict(pitch=(1 << 23) - 4), dict(pitch=1 << 23)) == [(FOUR, 0, 4096, 0, 0), generic]


def test_seven_waves_up_to_one_workgroup_per_compute_unit(plan):
    at = lambda s: dict(n_streams=s, blk_lanes=64)
    assert [g[0] for g in plan(at(64 * 256), at(64 * 256 + 1), at(64 * 256 + 64), [at(64 * 256), dict(cus=0)],
                               [at(64 * 256), dict(six_applicable=0)], [at(64 * 256 + 64), dict(policy=SEVEN_WAVE)])] == [SEVEN, FOUR, FOUR, FOUR, FOUR, SEVEN]
    # narrow groups count as workgroups: 2 048 streams in groups of 8 are 256, 2 056 are 257
    assert [g[0] for g in plan(SMALL, [SMALL, dict(n_streams=2056)])] == [SEVEN, FOUR]
    # calls of at least "stage_min_tiles" tiles (one 128-sample quantum); the pinned kernel takes shorter ones too
    assert plan([SMALL, dict(n=112)], [SMALL, dict(n=128)], [SMALL, dict(n=112, policy=SEVEN_WAVE)]) == [
        (FOUR, 0, 112, 0, 0), (SEVEN, 0, 128, 0, Y), (SEVEN, 0, 112, 0, Y)]
    # the half-tile counters' range holds for the pinned kernel as well
    short = dict(six_max_samples=1024)
    assert [g[0] for g in plan([SMALL, short, dict(n=1024)], [SMALL, short, dict(n=1040)], [SMALL, short, dict(n=1040, policy=SEVEN_WAVE)],
                               [SMALL, short, dict(n=1039)])] == [SEVEN, FOUR, FOUR, SEVEN]


def test_four_waves_beyond_one_round_need_two_slices(plan):
    big = dict(n_streams=81920, blk_queue=1, pipe_lds=30000)         # 1 280 groups on 1 024 resident workgroups, 5 per CU
    # 768 tiles are one slice: round 2's kernels -- two waves while five tiles fit a CU's LDS (and fewer than two waves per SIMD)
    assert [g[0] for g in plan([big, dict(n=768 * 16)], [big, dict(n=769 * 16)], [big, dict(n=768 * 16, pipe_lds=40000)],
                               [big, dict(n=768 * 16, policy=AUTO_R04)], [big, dict(n=768 * 16, policy=FOUR_WAVE)])] == [TWO, FOUR, ONE, TWO, FOUR]
    huge = dict(n_streams=262144, blk_queue=1)                       # 4 096 groups: four waves per SIMD
    assert [g[0] for g in plan([huge, dict(n=768 * 16)], [huge, dict(n=769 * 16)], [huge, dict(n=128)])] == [ONE, FOUR, ONE]
    # no queue or slicing off: never two slices; narrow groups are never beyond one round; "blk_min_tiles"
    assert [g[0] for g in plan([huge, dict(n=48000, blk_queue=0)], [huge, dict(n=48000, blk_slice_tiles=0xFFFFFFFF)],
                               [huge, dict(n=48000, blk_slice_tiles=100)], [huge, dict(n=128, blk_resident=4096)],
                               dict(n=128, blk_min_tiles=9), dict(n=144, blk_min_tiles=9))] == [ONE, ONE, FOUR, FOUR, TWO, FOUR]


def test_where_the_four_wave_kernel_does_not_apply(plan):
    # dsSPB not a multiple of four, or its LDS beyond a compute unit's: round 2's kernels; pinned: the next one down
    for off in (dict(blk_applicable=0), dict(blk_lds=LDS + 1)):
        assert [g[0] for g in plan(*[[off, dict(policy=p)] for p in range(7)])] == [TWO, TWO, TWO, TWO, TWO, TWO, ONE], off
    assert [g[0] for g in plan(dict(blk_lds=LDS))] == [FOUR]
    assert [g[0] for g in plan([SMALL, dict(blk_applicable=0)])] == [TWO]


def test_two_wave_lds_residency_rule(plan):
    r02 = dict(policy=AUTO_R02)                                      # 1 024 groups on 256 CUs: four tiles per CU
    assert [g[0] for g in plan([r02, dict(pipe_lds=LDS // 4)], [r02, dict(pipe_lds=LDS // 4 + 1)], dict(policy=TWO_WAVE, pipe_lds=LDS // 4 + 1),
                               dict(policy=TWO_WAVE, pipe_lds=LDS), dict(policy=TWO_WAVE, pipe_lds=LDS + 1))] == [TWO, ONE, TWO, TWO, ONE]
    # fewer than two waves per SIMD: under 8 groups per CU
    assert [g[0] for g in plan([r02, dict(n_streams=2047 * 64, pipe_lds=20000)], [r02, dict(n_streams=2048 * 64, pipe_lds=20000)],
                               [r02, dict(n_streams=2048 * 64, pipe_lds=20000, split_cus=257)])] == [TWO, ONE, TWO]


def test_exact_path_on_two_waves(plan):
    split2 = lambda *cases: [g[3] for g in plan(*[[F64, c] for c in cases])]
    assert plan([F64, dict(exact_split=1)]) == [(GENERIC, 0, 0, 1, 0)]
    assert split2(dict(exact_split=0), dict(exact_split=1), dict(exact_split=1, n=1)) == [0, 1, 1]
    small = lambda blocks, n: dict(exact_split=2, n_streams=64 * blocks, n=n)          # at most one group per SIMD, calls of >= 64 samples
    assert split2(small(1024, 64), small(1025, 64), small(1024, 63), small(1025, 63), dict(small(1024, 64), cus=0)) == [1, 0, 0, 0, 0]
    on = dict(exact_split=1)
    assert split2(dict(on, diagnostics=1), dict(on, wide_or_frac=1), dict(on, lock_step=0), dict(on, split2_lds=LDS), dict(on, split2_lds=LDS + 1)) == [0, 0, 0, 1, 0]
    assert plan(dict(exact_split=1, force_generic=1)) == [(GENERIC, 0, 0, 0, 0)]     # an fp32 engine's generic kernel: one wave


def test_host_stage_shift_is_three_exactly_where_the_head_is_odd(plan):
    def shift(f64, lock_step, parity):
        row = "shift=1,f64=%d,lock_step=%d,ds_parity=%d" % (f64, lock_step, parity)
        return int(subprocess.run([plan.exe, row], check=True, capture_output=True, text=True).stdout)
    assert [shift(f, l, p) for f in (0, 1) for l in (0, 1) for p in (0, 1)] == [0, 0, 0, 3, 0, 0, 0, 0]
    # ... which is where a lock-step fp32 engine's call starts with an odd head, whatever the policy and the ring's position
    for policy in range(7):
        for p in (0, 1):
            heads = [g[1] for g in plan(*[dict(policy=policy, ds_parity=p, ring_pos=r) for r in range(4)])]
            assert all(h % 2 == p for h in heads), (policy, p, heads)
            assert (shift(0, 1, p) == 3) == all(h % 2 == 1 for h in heads)
