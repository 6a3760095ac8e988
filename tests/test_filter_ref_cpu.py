"""tests/filter_ref.py, the CPU models the GPU filter tests compare against bit for bit, anchored without a GPU:

  * fma32 (the fp32 FIR's one-rounding multiply-add, emulated in float64) equals exact rational arithmetic rounded once to
    float32, on random triples and on triples built to land on and next to float32 halfway points -- among them sums whose
    float64 rounding is itself a halfway point with a non-zero error, where rounding twice goes wrong;
  * the FIR fp64 model equals the oracle's FIR and the recorded FIRFilter outputs of tests/golden; a cut into calls, a reset;
  * the IIR float64 model equals the oracle's IIR, the recorded process() doubles and the recorded processBuffer() floats."""
from fractions import Fraction

import numpy as np
import pytest

import filter_ref as fr
from conftest import golden


def _split(q):
    """|q| = (n + rest) ulp with n in [2^23, 2^24) and 0 <= rest < 1 (q a non-zero Fraction in float32's normal range)"""
    m = abs(q)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    assert Fraction(2) ** e <= m < Fraction(2) ** (e + 1) and -126 <= e <= 127
    ulp = Fraction(2) ** (e - 23)
    k = m / ulp
    n = k.numerator // k.denominator
    return n, k - n, ulp


def round_f32(q):
    """the Fraction q rounded once to float32, ties to even"""
    if q == 0:
        return np.float32(0.0)
    n, rest, ulp = _split(q)
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    v = float(n * ulp)                     # n <= 2^24: exact
    return np.float32(-v if q < 0 else v)


def _exact(a, b, c):
    return Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))


def exact_fma32(a, b, c):
    return round_f32(_exact(a, b, c))


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def test_round_f32_is_float32_rounding():
    r = np.random.default_rng(1)
    for v in fr.signed_uniform(r, 500, 2.0 ** -20, 2.0 ** 20):
        assert _bits(round_f32(Fraction(float(v)))) == _bits(np.float32(v))
    one, u = Fraction(1), Fraction(1, 2 ** 23)
    assert round_f32(one + u / 2) == np.float32(1.0)                              # a tie goes to the even neighbour
    assert round_f32(one + u + u / 2) == np.float32(1.0 + 2.0 ** -22)
    assert round_f32(one + u / 2 + Fraction(1, 2 ** 80)) == np.float32(1.0 + 2.0 ** -23)
    assert round_f32(-(one + u / 2 - Fraction(1, 2 ** 80))) == np.float32(-1.0)


def test_fma32_equals_exact_arithmetic_on_random_triples():
    r = np.random.default_rng(2)
    n = 4000
    a, b = (fr.signed_uniform(r, n).astype(np.float32) for _ in range(2))
    c = (fr.signed_uniform(r, n) * np.exp2(r.integers(-6, 7, n))).astype(np.float32)
    c[::7] = (-a[::7].astype(np.float64) * b[::7] * (1 + 2.0 ** -20)).astype(np.float32)     # heavy cancellation
    c[5::50] = 0.0
    got = fr.fma32(a, b, c)
    want = np.array([exact_fma32(*t) for t in zip(a, b, c)], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    assert _bits(fr.fma32(np.float32(0.5), a[:9], np.float32(0.0))).tolist() == _bits(np.float32(0.5) * a[:9]).tolist()   # a scalar tap


def _halfway_triples():
    """c a float32 (1 + j ulp) 2^E, the product +-(half an ulp of c) x (1 +- 2^-23)(1 +- 2^-23): exactly on a halfway point; off
    it by 2^-46 of half an ulp, which float64 cannot hold beside c (the float64 sum IS the halfway point, the error is not zero);
    and off it by 2^-22, which it can"""
    u = 2.0 ** -23
    for E in (0, 10, -7):
        for j in (0, 1, 2, 3, 2 ** 23 - 2, 2 ** 23 - 1):
            for cs in (1.0, -1.0):
                c = np.float32(cs * (1.0 + j * u) * 2.0 ** E)
                for ps in (1.0, -1.0):
                    for fa, fb in ((1.0, 1.0), (1 + u, 1 - u), (1 - u, 1 + u), (1 + u, 1 + u), (1 - u, 1 - u), (1 + u, 1.0), (1 - u, 1.0)):
                        yield np.float32(ps * fa * 2.0 ** (E - 24)), np.float32(fb), c
                        yield np.float32(ps * fa * 2.0 ** (E - 12)), np.float32(fb * 2.0 ** -12), c


def test_fma32_on_and_next_to_halfway_points():
    t = list(_halfway_triples())
    a, b, c = (np.array(v, np.float32) for v in zip(*t))
    got = fr.fma32(a, b, c)
    want = np.array([exact_fma32(*v) for v in t], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    twice = (a.astype(np.float64) * b + c).astype(np.float32)          # rounded to float64, then to float32
    exact_ties = sum(1 for v in t if _split(_exact(*v))[1] == Fraction(1, 2))
    assert np.count_nonzero(_bits(twice) != _bits(want)) >= 50         # the cases where the correction is what decides
    assert exact_ties >= 50                                            # true ties: they go to the even neighbour
    # both directions of the correction, and ties to even in both directions
    up = _bits(np.abs(want)) > _bits(np.abs(twice))
    down = _bits(np.abs(want)) < _bits(np.abs(twice))
    assert up.any() and down.any()


FIR_RUNS = [r for r in golden().manifest["filter_runs"] if isinstance(r["coeffs"], list)]
IIR_RUNS = [r for r in golden().manifest["filter_runs"] if isinstance(r["coeffs"], dict)]


@pytest.mark.parametrize("run", FIR_RUNS, ids=lambda r: r["name"])
def test_fir_fp64_model_equals_the_recorded_outputs(run):
    g = golden()
    x = g.array(run["x"])[None, :]
    want = g.array(run["y_buffer"])
    got = fr.FIRModel(run["coeffs"], 1, "f64").process_buffer(x)[0]
    assert np.array_equal(_bits(got), _bits(want))


def _x(seed, S, n):
    return fr.signed_uniform(np.random.default_rng(seed), (S, n)).astype(np.float32)


def test_fir_models_equal_the_oracle_in_calls_and_after_reset():
    from oracle import pyoracle as po
    S, n = 3, 300
    x = _x(3, S, n)
    for n_taps in (1, 2, 3, 4, 5, 8, 51, 130):
        taps = fr.signed_uniform(np.random.default_rng(100 + n_taps), n_taps)
        want = np.stack([po.FIR(list(taps)).process_buffer(x[s]) for s in range(S)])
        m = fr.FIRModel(taps, S, "f64")
        assert np.array_equal(_bits(m.process_buffer(x)), _bits(want)), n_taps
        whole32 = fr.FIRModel(taps, S, "f32").process_buffer(x)
        assert np.max(np.abs(whole32.astype(np.float64) - want)) <= n_taps * 2.0 ** -22 * 1.2 * 1.2   # (a sanity bound, not the check)
        for prec, whole in (("f64", want), ("f32", whole32)):
            # any cut into calls gives the whole; and from a reset delay line the output over a prefix is the prefix of the output
            m = fr.FIRModel(taps, S, prec)
            cuts = (0, 1, 4, 4 + max(0, n_taps - 2), 4 + 2 * max(0, n_taps - 2), 290, 290, n)
            parts = [m.process_buffer(x[:, p:q]) for p, q in zip(cuts, cuts[1:])]
            assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole)), (n_taps, prec)
            m.reset(1)
            again = m.process_buffer(x[:, :40])
            assert np.array_equal(_bits(again[1]), _bits(whole[1, :40]))              # stream 1 starts over
            if n_taps > 1:
                assert not np.array_equal(_bits(again[0]), _bits(whole[0, :40]))      # its neighbour carried on
            cont = fr.FIRModel(taps, S, prec)
            cont.process_buffer(x)
            assert np.array_equal(_bits(again[[0, 2]]), _bits(cont.process_buffer(x[:, :40])[[0, 2]]))
            m.reset()
            assert np.array_equal(_bits(m.process_buffer(x[:, :7])), _bits(whole[:, :7]))


@pytest.mark.parametrize("run", IIR_RUNS, ids=lambda r: r["name"])
def test_iir_float64_model_equals_the_recorded_outputs(run):
    g = golden()
    x = g.array(run["x"])
    co = run["coeffs"]
    m = fr.IIRModel(co["b"], co["a"], 1, "f64")
    got = m.process(x.astype(np.float64)[None, :], np.float64)[0]
    assert np.array_equal(got.view(np.uint64), g.array(run["y_process"]).view(np.uint64))       # process(): doubles
    m.reset()
    got = m.process(x[None, :], np.float32)[0]
    assert np.array_equal(_bits(got), _bits(g.array(run["y_buffer"])))                          # processBuffer(): Float32Array


def test_iir_float64_model_equals_the_oracle():
    from oracle import pyoracle as po
    S, n = 3, 120
    x = _x(4, S, n)
    r = np.random.default_rng(5)
    for nb, na, a0 in ((1, 1, 1.0), (2, 2, 1.25), (3, 3, 1.0), (9, 9, 0.8), (2, 1, 2.0), (1, 2, 1.0), (2, 4, 1.5), (9, 2, 1.0), (3, 9, 1.25)):
        b = list(fr.signed_uniform(r, nb))
        a = [a0] + list(fr.signed_uniform(r, na - 1, 2.0 ** -8, 0.4 / max(1, na - 1)))
        m = fr.IIRModel(b, a, S, "f64")
        y32 = m.process(x[:, :50], np.float32)
        y64 = m.process(x[:, 50:].astype(np.float64), np.float64)            # the two forms share the histories
        m.reset(2)
        z = m.process(x[:, :20], np.float32)
        for s in range(S):
            o = po.IIR(b, a)
            assert np.array_equal(_bits(y32[s]), _bits(o.process_buffer(x[s, :50]))), (nb, na, s)
            assert [o.process(float(v)) for v in x[s, 50:]] == y64[s].tolist(), (nb, na, s)
            if s == 2:
                o = po.IIR(b, a)
            assert np.array_equal(_bits(z[s]), _bits(o.process_buffer(x[s, :20]))), (nb, na, s)
