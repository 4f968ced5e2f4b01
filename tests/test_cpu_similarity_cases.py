"""tests/similarity_cases.py checked without a GPU: the integer oracle is exact (fractions.Fraction), the
fused and the unfused logit really differ on the shipped cases, every mutant of the kernel's tiling is
rejected, numpy-f32 accumulations stay within the derived logit bound and a dropped product does not, and
the exact softmax / sigmoid cases are what float64 says they are."""
import os

import numpy as np
import pytest

from tests import similarity_cases as cases
from tests.index_probs_cases import TINY, U, bound_matrix

F = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def test_the_shapes_cover_every_size_on_both_axes():
    assert {s[0] for s in cases.INT_SHAPES} == {1, 15, 16, 17, 33, 63, 64, 65, 129}
    assert {s[1] for s in cases.INT_SHAPES} == {1, 17, 64, 65, 130}
    assert {s[2] for s in cases.INT_SHAPES} == {16, 32, 80, 1152}
    assert {s[0] for s in cases.ROWS_KERNEL_SHAPES} == {1, 3, 4, 5, 9}
    assert {s[1] for s in cases.ROWS_KERNEL_SHAPES} == {1, 63, 64, 65, 200}
    assert {s[0] for s in cases.COLS_KERNEL_SHAPES} == {1, 2, 70}
    assert {s[1] for s in cases.COLS_KERNEL_SHAPES} == {1, 255, 256, 257}


@pytest.mark.parametrize("ni,nt,E", cases.INT_SHAPES)
def test_the_integer_oracle_is_exact_and_one_rounding(ni, nt, E):
    """|d| < 2^24 (so the f32 dot is exact in any order), the float64 expression equals the rational value
    on a sample of every case, and the model of the kernel's tiling without a mutant is the oracle."""
    a, b = cases.int_case(ni, nt, E)
    assert np.abs(a).max() <= 8 and np.abs(b).max() <= 8
    d = cases.int_dot(a, b)
    assert (np.abs(a.astype(np.int64)) @ np.abs(b.astype(np.int64)).T).max() < 2 ** 24  # every partial sum
    rng = np.random.default_rng(ni + nt + E)
    sample = d.ravel()[rng.integers(0, d.size, 40)]
    for scale, bias in cases.PAIRS:
        assert all(cases.float64_is_exact(x, scale, bias) for x in sample), (scale, bias)
        want = cases.logits_oracle(a, b, scale, bias)
        assert want.dtype == F and want.shape == (ni, nt)
        assert np.array_equal(bits(cases.model(a, b, scale, bias)), bits(want))


@pytest.mark.parametrize("E", [16, 80, 1152])
@pytest.mark.parametrize("scale,bias", [(117.33, -12.9), (100.0, 0.0), (100.0, -16.5), (0.37, 3.1)])
def test_float64_is_exact_at_the_extremes(E, scale, bias):
    for d in (64 * E, -64 * E, 64 * E - 1, 1, -1, 0, 12345 % (64 * E)):
        assert cases.float64_is_exact(d, scale, bias)


@pytest.mark.parametrize("ni,nt,E", cases.INT_SHAPES)
@pytest.mark.parametrize("scale,bias", cases.FUSED_PAIRS)
def test_two_roundings_differ_from_one_on_every_shipped_case(ni, nt, E, scale, bias):
    a, b = cases.int_case(ni, nt, E)
    d = cases.int_dot(a, b)
    share = np.mean(bits(cases.two_roundings(d, scale, bias)) != bits(cases.fused(d, scale, bias)))
    assert share >= 0.10, share


def test_one_and_two_roundings_agree_where_the_product_is_exact():
    """(100, 0): |100 d| < 2^24 is an integer, so this pair says nothing about the fmaf; it is shipped for
    the index's own scale."""
    a, b = cases.int_case(129, 130, 80)
    d = cases.int_dot(a, b)
    assert np.array_equal(bits(cases.two_roundings(d, 100.0, 0.0)), bits(cases.fused(d, 100.0, 0.0)))


@pytest.mark.parametrize("mutant", cases.MUTANTS)
def test_every_mutant_is_rejected_on_the_integer_cases(mutant):
    applied = 0
    for ni, nt, E in cases.INT_SHAPES:
        a, b = cases.int_case(ni, nt, E)
        for pair in cases.PAIRS:
            if not cases.mutant_applies(mutant, ni, nt, pair):
                continue
            applied += 1
            want = cases.logits_oracle(a, b, *pair)
            assert not np.array_equal(bits(cases.model(a, b, *pair, mutant=mutant)), bits(want)), (ni, nt, E, pair)
    assert applied >= 12


@pytest.mark.parametrize("mutant", [m for m in cases.MUTANTS if m != "two roundings"])
def test_the_stamp_and_the_census_reject_the_structural_mutants(mutant):
    for ni, nt in cases.STAMP_SHAPES:
        a, b = cases.stamp_case(ni, nt)
        assert cases.stamp_diff(cases.model(a, b, 1.0, 0.0), ni, nt) is None
        if mutant != "last slab dropped":  # E = 16 is one slab; the census below has more
            msg = cases.stamp_diff(cases.model(a, b, 1.0, 0.0, mutant=mutant), ni, nt)
            assert msg is not None and "<-" in msg
    for E in cases.CENSUS_E:
        a, b = cases.census_case(E)
        want = cases.census_expected(E)
        assert np.array_equal(bits(cases.model(a, b, 1.0, 0.0)), bits(want))
        assert np.array_equal(bits(cases.logits_oracle(a, b, 1.0, 0.0)), bits(want))
        assert not np.array_equal(bits(cases.model(a, b, 1.0, 0.0, mutant=mutant)), bits(want)), E


def test_the_stamp_is_exact_and_decodes():
    for ni, nt in cases.STAMP_SHAPES:
        a, b = cases.stamp_case(ni, nt)
        want = cases.stamp_expected(ni, nt)
        assert want.max() < 2 ** 24 and len(np.unique(want)) == ni * nt
        assert np.array_equal(bits(cases.logits_oracle(a, b, 1.0, 0.0)), bits(want))
        assert cases.stamp_decode(want[ni - 1, nt - 1]) == (ni - 1, nt - 1)
        assert cases.stamp_decode(want[0, 64]) == (0, 64)
    swapped = cases.stamp_expected(130, 200)
    swapped[[3, 70]] = swapped[[70, 3]]
    msg = cases.stamp_diff(swapped, 130, 200)
    assert msg.startswith("400 wrong") and "(3, 0) <- (70, 0)" in msg
    assert cases.stamp_decode(F(np.nan)) != cases.stamp_decode(F(np.nan))  # a NaN is reported as itself


# ---- the derived bound for real-valued logits --------------------------------------------------------------
@pytest.mark.parametrize("E", cases.UNIT_E)
@pytest.mark.parametrize("scale,bias", cases.BOUND_PAIRS)
def test_f32_accumulations_stay_within_the_logit_bound_and_a_dropped_product_does_not(E, scale, bias):
    a, b = cases.unit_case(E, 20, 30)
    ref, mags = cases.logits64(a, b, scale, bias)
    bound = cases.logit_bound(E, scale, mags, ref)
    seq, pair = cases.dot_sequential(a, b), cases.dot_pairwise4(a, b)
    assert not np.array_equal(bits(seq), bits(pair))  # two different orders
    for acc in (seq, pair):
        err = np.abs(cases.epilogue(acc, scale, bias).astype(np.float64) - ref)
        assert (err <= bound).all(), float((err / bound).max())
    err = np.abs(cases.epilogue(cases.dot_sequential(a, b, drop=0), scale, bias).astype(np.float64) - ref)
    assert np.mean(err > bound) > 0.5, float(np.mean(err > bound))


# ---- softmax and sigmoid -----------------------------------------------------------------------------------
def f32_softmax(L, axis):
    """A plain f32 softmax (expf within half an ulp, sequential sum)."""
    L = np.moveaxis(np.asarray(L, F), axis, 0)
    m = np.fmax.reduce(L, axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((L - m).astype(np.float64)).astype(F)
        s = np.zeros_like(m)
        for row in e:
            s = s + row
        return np.moveaxis(e / s, 0, axis)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("scale", cases.SOFTMAX_SCALES)
def test_check_softmax_accepts_an_f32_softmax_and_rejects_mistakes(axis, scale):
    a, b = cases.unit_case(64, 9, 200) if axis == 1 else cases.unit_case(64, 70, 257)
    L = cases.logits64(a, b, scale, 0.0)[0].astype(F)  # stands in for the device's logits
    p = f32_softmax(L, axis)
    cases.check_softmax(p, L, axis)
    other = f32_softmax(L, 1 - axis)  # the wrong axis
    with pytest.raises(AssertionError):
        cases.check_softmax(other, L, axis)
    bumped = p * F(1 + 2.0 ** -10)  # a few thousand ulps
    with pytest.raises(AssertionError):
        cases.check_softmax(bumped.astype(F), L, axis)
    nomax = np.exp(L.astype(np.float64))  # no max subtraction, but otherwise right: accepted while finite
    if scale == 1.0:
        cases.check_softmax((nomax / nomax.sum(axis=axis, keepdims=True)).astype(F), L, axis)


def test_check_softmax_treats_nan_and_inf_as_the_oracle_does():
    L = np.zeros((3, 5), F)
    L[1, 2] = np.inf
    L[2, 0] = np.nan
    p, R, n = cases.softmax_oracle(L, 1)
    assert (p[0] == 0.2).all() and np.isnan(p[1:]).all() and R == 0.0 and n == 5
    p0, _, n0 = cases.softmax_oracle(L, 0)
    assert np.isnan(p0[:, [0, 2]]).all() and (p0[:, [1, 3, 4]] == 1 / 3).all() and n0 == 3
    cases.check_softmax(p.astype(F), L, 1)
    with pytest.raises(AssertionError):
        cases.check_softmax(np.nan_to_num(p, nan=0.2).astype(F), L, 1)


@pytest.mark.parametrize("ni,nt,axis", cases.PATTERN_SHAPES)
def test_the_pattern_cases_have_exact_softmaxes(ni, nt, axis):
    a, b, L = cases.pattern_case(ni, nt, axis)
    assert np.array_equal(bits(cases.logits_oracle(a, b, cases.PATTERN_SCALE, 0.0)), bits(L))
    assert not np.signbit(L).any() or (L[np.signbit(L)] == -128).all()  # the zeros are +0
    assert np.exp(-128.0) < 2.0 ** -150  # expf(-128) rounds to 0, flushed or not
    p = cases.exact_softmax(L, axis)
    ref, R, n = cases.softmax_oracle(L, axis)
    assert np.abs(p - ref).max() <= U * ref.max() + n * np.exp(-128.0)
    lines = np.moveaxis(L, axis, 1)
    probs = np.moveaxis(p, axis, 1)
    assert (lines[0] == 0).sum() == 1 and probs[0].max() == 1.0 and probs[0].sum() == 1.0  # a single zero
    assert (lines[1] == -128).all() and np.array_equal(bits(probs[1]), bits(np.full(n, F(1) / F(n))))  # all equal
    counts = (lines == lines.max(axis=1, keepdims=True)).sum(axis=1)
    assert len(np.unique(counts)) >= min(len(lines), n, 4)  # the lines differ, so a mix-up changes the answer
    if min(ni, nt) > 1:
        assert not np.array_equal(bits(cases.exact_softmax(L, 1 - axis)), bits(p))
    assert np.array_equal(bits(f32_softmax(L, axis)), bits(p))


def test_the_sigmoid_bound_and_the_saturation_case():
    a, b, want = cases.saturation_case()
    L = cases.logits_oracle(a, b, 128.0, 0.0)
    assert set(np.unique(L)) == {-128.0, 0.0, 128.0}
    for l, v in ((0.0, 0.5), (128.0, 1.0), (-128.0, 0.0)):
        assert (want[L == l] == v).all() and (L == l).sum() >= 10
    assert (want[0] == 0.5).all() and set(want[1]) == {0.5, 1.0} and set(want[2]) == {0.5, 0.0}
    with np.errstate(over="ignore"):
        f32 = F(1) / (F(1) + np.exp(-L.astype(np.float64)).astype(F))
    assert np.array_equal(bits(f32), bits(want))
    cases.check_sigmoid(want, L)
    x = np.linspace(-100, 100, 4001).astype(F)[None, :]
    with np.errstate(over="ignore"):
        p = (F(1) / (F(1) + np.exp(-x.astype(np.float64)).astype(F))).astype(F)
    cases.check_sigmoid(p, x)
    with pytest.raises(AssertionError):
        cases.check_sigmoid((p * F(1 + 2.0 ** -20)).astype(F), x)  # four ulps
    assert cases.SIGMOID_BOUND < 2.0 ** -21 and TINY == 2.0 ** -126
    assert bound_matrix(200, 200.0) < 2.0 ** -14


def test_the_cases_module_imports_without_the_library():
    import subprocess
    import sys
    code = ("import sys, tests.similarity_cases; "
            "assert not any(m.startswith(('open_clip_inference', 'torch')) for m in sys.modules)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], cwd=root, check=True)


def test_the_size_refusals_need_no_device():
    """check_similarity_args runs before anything touches the GPU: more image rows than launch_similarity's
    grid holds (65535 * 64) is the Shape error of the other size checks, in both entry points."""
    from open_clip_inference import _lib
    from open_clip_inference.error import ShapeError
    L = _lib.lib()
    p = np.zeros(16, F).ctypes.data
    for rows in (65535 * 64 + 1, 1 << 22, 1 << 23):
        for rc in (L.clipgpu_similarity_device(p, rows, p, 1, 16, 1.0, 0.0, 2, 1, p, None),
                   L.clipgpu_similarity(0, p, rows, p, 1, 16, 1.0, 0.0, 2, 1, p)):
            assert rc != 0
            with pytest.raises(ShapeError, match="Shape error: similarity matrix too large"):
                _lib.check(rc)
    assert L.clipgpu_similarity_device(p, 1, p, 1, 24, 1.0, 0.0, 2, 1, p, None) != 0
    assert b"Shape error: embedding dim must be a multiple of 16" in L.clipgpu_last_error()
