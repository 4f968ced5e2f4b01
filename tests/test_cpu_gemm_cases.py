"""The exact references of tests/test_gpu_gemm.py, checked without a GPU (tests/gemm_cases.py), for every
case the GPU file runs:
  * the exactness precondition: sum |a||w| + |bias| < 2^24 for every element, finite f16 outputs, and the
    accumulator re-summed as an f32 chain over shuffled 32-wide K blocks gives the same bits;
  * agreement with fp64: the f32-ordered reference is within 2^-23 relative per add, plus one output
    rounding, of the fp64 result;
  * mutants of the reference: exact inputs must also discriminate.  Each mutant -- a bug an epilogue or a
    tile walk could have -- must change at least 95 % of the elements it can affect.  Where a case falls
    short the inputs change, never the share."""
import numpy as np
import pytest

from tests import gemm_cases as gc
from tests.gemm_cases import BF16, F16

SHARE = 0.95
TYPES = [BF16, F16]
TYPE_IDS = ["bf16", "f16"]

# (M, N, K, modes): every dense case of the GPU file (the pitch case is SHAPES[1]; the walk runs mode 3)
DENSE = [(M, N, K, gc.MODES) for M, N, K in gc.SHAPES] + [(M, N, K, [0]) for M, N, K in gc.GENERAL_SHAPES] + \
    [gc.WALK_SHAPE + ([gc.WALK_MODE],)]
DENSE_IDS = ["x".join(map(str, d[:3])) for d in DENSE]


def changed(mut, ref, rows=slice(None)):
    return float(np.mean(mut[rows] != ref[rows]))


def check_precondition(A, W, bias, extra=0.0):
    terms = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T
    if bias is not None:
        terms = terms + np.abs(bias).astype(np.float64)
    assert terms.max() < 2 ** 24
    assert terms.max() <= 16 * A.shape[1] + (0 if bias is None else np.abs(bias).max())
    return terms + extra


@pytest.mark.parametrize("M,N,K,modes", DENSE, ids=DENSE_IDS)
def test_dense_cases_are_exact_and_agree_with_fp64(M, N, K, modes):
    c = gc.gemm_case(M, N, K)
    assert np.all(np.abs(c.A) <= 4) and np.all(c.A == np.rint(c.A)) and np.all(np.abs(c.W) <= 4)
    assert len(np.unique(c.bias)) == N and np.all(c.bias != 0)
    shuffled = gc.shuffled_block_acc(c.A, c.W, seed=M + N)
    assert np.array_equal(shuffled, gc.acc_of(c.A, c.W).astype(np.float32))
    walk = (M, N, K) == gc.WALK_SHAPE  # (17 M elements: the one type and bias form the GPU file runs)
    for mode in modes:
        for dtype in [gc.WALK_TYPE] if walk else TYPES:
            for bias in [True] if walk else [True, False]:
                ref = c.ref(mode, dtype, bias)
                assert np.all(np.isfinite(ref))
                ot = gc.out_type(mode, dtype)
                # the same epilogue on the shuffled f32 chain: the same bits
                again = gc.epilogue(shuffled.astype(np.int64), c.bias if bias else None, c.x(mode), ot)
                assert np.array_equal(again.view(np.uint32), ref.view(np.uint32))
                x = c.x(mode)
                terms = check_precondition(c.A, c.W, c.bias if bias else None, 0.0 if x is None else np.abs(x))
                r64 = c.ref64(mode, bias)
                assert np.all(np.abs(ref - r64) <= gc.f64_bound(r64, terms, ot)), (mode, dtype)
    if 3 in modes:  # the f16-stream results are mostly not representable before the rounding
        v = gc.epilogue(gc.acc_of(c.A, c.W), c.bias, c.resid16, "f32")
        assert np.mean(v != c.ref(3, BF16)) > 0.9


@pytest.mark.parametrize("M,N,K,modes", DENSE, ids=DENSE_IDS)
def test_dense_cases_reject_the_mutants(M, N, K, modes):
    c = gc.gemm_case(M, N, K)
    for mode in modes:
        for dtype in [gc.WALK_TYPE] if (M, N, K) == gc.WALK_SHAPE else TYPES:
            ref = c.ref(mode, dtype)
            share = {"last 32 of K dropped": changed(c.ref(mode, dtype, A=c.A[:, :-32], W=c.W[:, :-32]), ref)}
            ot = gc.out_type(mode, dtype)
            rolled = gc.epilogue(gc.acc_of(c.A, c.W), np.roll(c.bias, 4), c.x(mode), ot)
            share["bias rolled by 4 columns"] = changed(rolled, ref)
            if M > 1:  # (one row: no neighbour)
                share["rows shifted by one"] = changed(np.roll(ref, 1, axis=0), ref)
                if mode in (1, 3):
                    neighbour = np.roll(c.x(mode), 1, axis=0)
                    share["resid of the neighbouring row"] = changed(c.ref(mode, dtype, x=neighbour), ref)
            for name, s in share.items():
                assert s >= SHARE, (name, mode, dtype, s)


def test_rounding_case_rejects_two_roundings():
    """result -> f16 -> bf16 against the single rounding, on the case built for it."""
    c = gc.rounding_case()
    check_precondition(c.A, c.W, c.bias)
    acc = gc.acc_of(c.A, c.W)
    assert np.mean((np.abs(acc) >= 128) & (np.abs(acc) < 256)) > 0.97
    ref = c.ref(0, BF16)
    v = gc.epilogue(acc, c.bias, None, "f32")
    twice = gc.round16(gc.round16(v, F16), BF16)
    assert changed(twice, ref) >= SHARE
    assert np.array_equal(gc.epilogue(gc.shuffled_block_acc(c.A, c.W, 3).astype(np.int64), c.bias, None, BF16), ref)
    r64 = acc + c.bias.astype(np.float64)
    assert np.all(np.abs(ref - r64) <= gc.f64_bound(r64, np.abs(r64) + 1, BF16))


@pytest.mark.parametrize("B,G,Kp,D", gc.PATCH_SHAPES, ids=["x".join(map(str, s)) for s in gc.PATCH_SHAPES])
@pytest.mark.parametrize("cls", [0, 1])
def test_patch_cases(cls, B, G, Kp, D):
    c = gc.patch_case(cls, B, G, Kp, D)
    assert len(np.unique(c.pos, axis=0)) == c.tokens and len(np.unique(c.bias)) == D
    shuffled = gc.shuffled_block_acc(c.rows, c.W, seed=D)
    assert np.array_equal(shuffled, gc.acc_of(c.rows, c.W).astype(np.float32))
    m = np.arange(B * c.G2)
    for x16 in (0, 1):
        for bias in (True, False):
            ref = c.ref(x16, bias)
            assert np.all(np.isfinite(ref))
            if cls:  # the class rows keep the sentinel
                assert np.all(ref[np.arange(B) * c.tokens] == gc.SENTINEL)
            got = c.patch_rows_of(ref)
            assert not np.any(got == gc.SENTINEL)
            pos = c.pos[cls + m % c.G2]
            terms = check_precondition(c.rows, c.W, c.bias if bias else None, np.abs(pos))
            r64 = c.ref64(bias)
            assert np.all(np.abs(got - r64) <= gc.f64_bound(r64, terms, F16 if x16 else "f32"))
            again = gc.epilogue(shuffled.astype(np.int64), c.bias if bias else None, pos, F16 if x16 else "f32")
            assert np.array_equal(again, got)
        ref = c.ref(x16)
        full = PatchMutants(c, x16)
        share = {"last 32 of K dropped": changed(full.drop_k(), ref, full.patch_rows),
                 "bias rolled by 4 columns": changed(full.roll_bias(), ref, full.patch_rows)}
        if B * c.G2 > 1:
            share["rows shifted by one"] = changed(full.shift_rows(), ref, full.patch_rows)
        if cls:
            share["pos taken at p"] = changed(c.ref(x16, pos_shift=0), ref, full.patch_rows)
            # image 0 stays in place; image b >= 1 lands b rows early: the rows either form writes for it
            late = m[m >= c.G2]
            later = np.union1d(full.patch_rows[late], late // c.G2 * c.G2 + cls + late % c.G2)
            share["token row computed with G^2"] = changed(c.ref(x16, row_tokens=c.G2), ref, later)
        for name, s in share.items():
            assert s >= SHARE, (name, x16, s)


class PatchMutants:
    def __init__(self, c, x16):
        self.c, self.x16 = c, x16
        m = np.arange(c.B * c.G2)
        self.patch_rows = m // c.G2 * c.tokens + c.cls + m % c.G2

    def variant(self, **changes):
        d = gc.PatchCase.__new__(gc.PatchCase)
        d.__dict__.update(self.c.__dict__)
        d.__dict__.update(changes)
        return d.ref(self.x16)

    def drop_k(self):
        return self.variant(rows=self.c.rows[:, :-32], W=self.c.W[:, :-32])

    def roll_bias(self):
        return self.variant(bias=np.roll(self.c.bias, 4))

    def shift_rows(self):
        out = self.c.ref(self.x16)
        out[self.patch_rows] = np.roll(out[self.patch_rows], 1, axis=0)
        return out


@pytest.mark.parametrize("M,N,K", gc.MX_SHAPES)
def test_mx_cases(M, N, K):
    """The MX operands are the integers exactly (MxCase asserts it), under one scale; the reference and
    its mutants as the dense cases'."""
    c = gc.mx_case(M, N, K)
    shuffled = gc.shuffled_block_acc(c.A, c.W, seed=K)
    for mode in gc.MX_MODES:
        for dtype in TYPES:
            ref = c.ref(mode, dtype)
            ot = gc.mx_out_type(mode, dtype)
            assert np.all(np.isfinite(ref))
            assert np.array_equal(gc.epilogue(shuffled.astype(np.int64), c.bias, c.x(mode), ot), ref)
            x = c.x(mode)
            terms = check_precondition(c.A, c.W, c.bias, 0.0 if x is None else np.abs(x))
            r64 = gc.acc_of(c.A, c.W) + c.bias.astype(np.float64) + (0.0 if x is None else x.astype(np.float64))
            assert np.all(np.abs(ref - r64) <= gc.f64_bound(r64, terms, ot))
            acc, acc_short = gc.acc_of(c.A, c.W), gc.acc_of(c.A[:, :-32], c.W[:, :-32])
            share = {"last 32 of K dropped": changed(gc.epilogue(acc_short, c.bias, x, ot), ref),
                     "rows shifted by one": changed(np.roll(ref, 1, axis=0), ref),
                     "bias rolled by 4 columns": changed(gc.epilogue(acc, np.roll(c.bias, 4), x, ot), ref)}
            if x is not None:
                neighbour = gc.epilogue(acc, c.bias, np.roll(x, 1, axis=0), ot)
                share["resid of the neighbouring row"] = changed(neighbour, ref)
            for name, s in share.items():
                assert s >= SHARE, (name, mode, dtype, s)
