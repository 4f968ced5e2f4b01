"""Inputs, oracles, bounds and mutants for the similarity kernels (csrc/kernels/similarity.hip:
sim_logits_kernel, softmax_rows_kernel, softmax_cols_kernel, reached through clipgpu_similarity and
clipgpu_similarity_device).  tests/test_cpu_similarity_cases.py shows on the CPU that the oracles are right
and reject the mutants; tests/test_gpu_similarity.py holds the kernels to them.  No GPU import.

These kernels are what the embedding index's tests take as their expected result bit for bit, so the parts
that can be exact are exact:

1. Logits on integer operands.  With img, txt integers in [-8, 8] and E <= 1152 every product and every
   partial sum of a dot is an integer of magnitude <= 64 * 1152 < 2^24: the f32 accumulator of the MFMA is
   exact in any order, and the output bits are determined by the one fmaf the kernel's header promises,
       out[i][j] = round_f32(d * scale + bias),     d the integer dot, scale and bias as f32.
   logits_oracle computes d in int64 and d * float64(scale) + float64(bias) in float64: d has <= 17 bits and
   an f32 scale 24, so the product is exact (<= 41 bits), and so is the sum with an f32 bias at the
   magnitudes here (it fits in 53 bits; the CPU test compares with fractions.Fraction).  One rounding to
   f32 follows.  A logit built as f32(f32(d) * scale) + bias (two roundings) differs from that on about
   30 % of the elements for the pairs FUSED_PAIRS.
   Structure: the coordinate stamp writes (i + 1) + 1024 (j + 1) into out[i][j], so that a moved tile reads
   as a wrong coordinate; the K census (img = identity, txt[j][k] = k + 1 + j) counts every k position
   once with weight one.
   model() is the kernel's tiling restated on integers (64 x 64 blocks, rows and columns past the end
   staged as copies of the last one, TK = 16 slabs) with one mistake each: MUTANTS.

2. Real-valued logits (unit rows).  The dot is E products a_k b_k accumulated by fmaf in some order: one
   rounding per product, each of a partial sum no larger than sum_k |a_k b_k|.  So
       |acc - d| <= (E u / (1 - E u)) sum_k |a_k b_k|,                 u = 2^-24,
   and out = fmaf(acc, scale, bias) = (acc scale + bias)(1 + e), |e| <= u, gives
       |out - ref64| <= |scale| |acc - d| (1 + u) + u |ref64|
                     <= HI (E u |scale| sum_k |a_k b_k| + u |ref64|),  HI = 1 + 2^-11 >= (1 + u) / (1 - E u)
   for E <= 1152 (E u < 2^-13).  (No product or partial sum of unit rows comes near 2^-126.)  This is
   logit_bound.  tests/gemm_cases.py has f64_bound, but that bounds the two epilogue adds behind an exact
   accumulator, not K roundings, so it does not serve here.  The bound is loose by nature (it allows E
   worst-case roundings); part 1 and the position-independence tests carry the precision, this one catches
   an accumulation that loses more than rounding, such as a dropped product.

3. Softmax and sigmoid are held on the kernels' own f32 logits L (a "logits" call), against float64:
   softmax within index_probs_cases.bound_matrix(n, R) relative plus TINY, every row (column) summing to 1
   within n u (to first order: at most n - 1 adds and one division, each within u; the strided chain plus
   tree of the rows kernel does fewer); sigmoid 1 / (1 + expf(-l)) within HI (ue + 2 u) relative plus TINY
   (one expf, one add, one IEEE division).  Where the logits of a row take only the values 0 and -128,
   expf gives exactly 1 and 0 (e^-128 < 2^-150 rounds to 0), the sum is a small integer c, and every
   probability is exactly f32(1) / f32(c) or 0: exact_softmax."""
import functools
from fractions import Fraction

import numpy as np

from tests.index_cases import unit_rows
from tests.index_probs_cases import HI, TINY, U, UE, bound_matrix, oracle as softmax_rows_oracle

F = np.float32
TB, TK = 64, 16  # similarity.hip: block edge, K slab

# ---- 1. integer operands ---------------------------------------------------------------------------------
FUSED_PAIRS = [(117.33, -12.9), (0.37, 3.1)]  # one rounding and two roundings differ on ~30 % of elements
PAIRS = FUSED_PAIRS + [(100.0, 0.0)]
# every ni of {1, 15, 16, 17, 33, 63, 64, 65, 129} and nt of {1, 17, 64, 65, 130}; every E with a ragged shape
INT_SHAPES = [(1, 130, 16), (15, 17, 32), (16, 64, 80), (17, 65, 1152), (33, 1, 16), (63, 130, 32), (64, 1, 80),
              (65, 17, 1152), (129, 64, 16), (129, 130, 80), (65, 65, 1152), (64, 64, 32)]
STAMP_SHAPES = [(130, 200), (200, 130)]
CENSUS_E = [16, 80, 1152]
CENSUS_NT = 70


@functools.lru_cache(maxsize=None)
def int_case(ni, nt, E):
    """Seeded integers in [-8, 8] as f32: (img [ni][E], txt [nt][E]); shared, never written to."""
    rng = np.random.default_rng([ni, nt, E])
    a, b = (rng.integers(-8, 9, size=(n, E)).astype(F) for n in (ni, nt))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def int_dot(a, b):
    """int64 a . b^T of integer-valued f32 matrices."""
    ai, bi = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    assert np.array_equal(ai, a) and np.array_equal(bi, b)
    return ai @ bi.T


def fused(d, scale, bias):
    """round_f32(d * scale + bias) for an int64 d with |d| < 2^24 and f32 scale, bias: exact in float64."""
    assert np.abs(d).max() < 2 ** 24
    return (d.astype(np.float64) * np.float64(F(scale)) + np.float64(F(bias))).astype(F)


def two_roundings(d, scale, bias):
    """f32(f32(d) * scale) + bias in f32: what the logit is without the fmaf."""
    r = (d.astype(F) * F(scale)).astype(F) + F(bias)
    assert r.dtype == F
    return r


def logits_oracle(a, b, scale, bias):
    return fused(int_dot(a, b), scale, bias)


def float64_is_exact(d, scale, bias):
    """Whether d * float64(scale) + float64(bias), as fused() evaluates it, is the exact rational value, so
    that the cast to f32 is the only rounding."""
    v = np.float64(int(d)) * np.float64(F(scale)) + np.float64(F(bias))
    return Fraction(float(v)) == Fraction(int(d)) * Fraction(float(F(scale))) + Fraction(float(F(bias)))


def stamp_case(ni, nt):
    """img[i] = (i + 1, 1, 0, ...), txt[j] = (1, 1024 (j + 1), 0, ...): out[i][j] = (i + 1) + 1024 (j + 1) at
    scale 1, bias 0."""
    a, b = np.zeros((ni, 16), F), np.zeros((nt, 16), F)
    a[:, 0], a[:, 1] = np.arange(1, ni + 1), 1
    b[:, 0], b[:, 1] = 1, 1024 * np.arange(1, nt + 1)
    return a, b


def stamp_expected(ni, nt):
    return (np.arange(1, ni + 1)[:, None] + 1024 * np.arange(1, nt + 1)[None, :]).astype(F)


def stamp_decode(v):
    """The (i, j) a stamped value names, or the value itself if it names none."""
    if not np.isfinite(v) or v != int(v) or v < 1025:
        return float(v)
    return int(v) % 1024 - 1, int(v) // 1024 - 1


def stamp_diff(got, ni, nt):
    """None if got is the stamp; else a message that names the first wrong elements and what they hold."""
    want = stamp_expected(ni, nt)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad) == 0:
        return None
    return f"{len(bad)} wrong of {ni * nt}; (i, j) holds: " + ", ".join(
        f"({i}, {j}) <- {stamp_decode(got[i, j])}" for i, j in bad[:8])


def census_case(E, nt=CENSUS_NT):
    """img = identity [E][E], txt[j][k] = k + 1 + j: out[i][j] = i + 1 + j at scale 1, bias 0."""
    a = np.eye(E, dtype=F)
    b = (np.arange(E)[None, :] + 1 + np.arange(nt)[:, None]).astype(F)
    return a, b


def census_expected(E, nt=CENSUS_NT):
    return (np.arange(E)[:, None] + 1 + np.arange(nt)[None, :]).astype(F)


MUTANTS = ["last slab dropped", "slab twice", "clamp leak", "quadrants swapped", "two roundings"]


def mutant_applies(mutant, ni, nt, pair=None):
    """Whether the mistake can show at this shape / (scale, bias) at all."""
    if mutant == "clamp leak":  # needs staged rows or columns past the end
        return ni % TB != 0 or nt % TB != 0
    if mutant == "quadrants swapped":  # rows 0..31 x cols 32..63 <-> rows 32..63 x cols 0..31 of a block
        return ni > 32 or nt > 32
    if mutant == "two roundings":
        return pair is None or tuple(pair) in FUSED_PAIRS
    return True


def model(a, b, scale, bias, mutant=None):
    """sim_logits_kernel restated on integers: blocks of 64 x 64 over rows and columns staged with the
    kernel's clamp (min(i, ni - 1)), K in slabs of 16, the fused epilogue, the bounds-checked store; with
    `mutant`, one mistake."""
    ni, nt, E = len(a), len(b), a.shape[1]
    pi, pj = -(-ni // TB) * TB, -(-nt // TB) * TB
    A = np.asarray(a).astype(np.int64)[np.minimum(np.arange(pi), ni - 1)]
    B = np.asarray(b).astype(np.int64)[np.minimum(np.arange(pj), nt - 1)]
    slabs = list(range(0, E, TK))
    if mutant == "last slab dropped":
        slabs = slabs[:-1]
    if mutant == "slab twice":
        slabs = slabs + slabs[:1]
    d = np.zeros((pi, pj), np.int64)
    for k0 in slabs:
        d += A[:, k0:k0 + TK] @ B[:, k0:k0 + TK].T
    if mutant == "clamp leak":  # the first copy of the last row / column is added into it instead of dropped
        if pi > ni:
            d[ni - 1, :] += d[ni, :]
        if pj > nt:
            d[:, nt - 1] += d[:, nt]
    if mutant == "quadrants swapped":
        t = d.reshape(pi // TB, TB, pj // TB, TB)
        top = t[:, :32, :, 32:].copy()
        t[:, :32, :, 32:] = t[:, 32:, :, :32]
        t[:, 32:, :, :32] = top
    d = d[:ni, :nt]
    return two_roundings(d, scale, bias) if mutant == "two roundings" else fused(d, scale, bias)


# ---- 2. unit rows: position independence and the derived bound -------------------------------------------
UNIT_NI, UNIT_NT = 70, 130
UNIT_E = [64, 1152]
BOUND_PAIRS = [(100.0, 0.0), (10.0, -10.0)]


@functools.lru_cache(maxsize=None)
def unit_case(E, ni=UNIT_NI, nt=UNIT_NT):
    """Seeded L2-normalised Gaussian rows: (img [ni][E], txt [nt][E]); shared, never written to."""
    rng = np.random.default_rng([7000, ni, nt, E])
    a, b = unit_rows(rng, ni, E), unit_rows(rng, nt, E)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def logits64(a, b, scale, bias):
    """(ref64, sum_k |a_k b_k|), both [ni][nt] float64."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a64 @ b64.T * np.float64(F(scale)) + np.float64(F(bias)), np.abs(a64) @ np.abs(b64).T


def logit_bound(E, scale, mags, ref64):
    assert E * U < 2.0 ** -13
    return HI * (E * U * abs(float(F(scale))) * mags + U * np.abs(ref64))


def fma_step(acc, x, y):
    """f32 fmaf(x, y, acc) elementwise: the float64 product of two f32 is exact, the sum is rounded to 53
    bits and then to 24, which differs from one rounding only on a 2^-29 share of near-ties."""
    return (acc.astype(np.float64) + x.astype(np.float64) * y.astype(np.float64)).astype(F)


def dot_sequential(a, b, drop=None):
    """acc = fmaf(a_k, b_k, acc) for k ascending, in f32; `drop`: a k that is left out (the mutant)."""
    acc = np.zeros((len(a), len(b)), F)
    for k in range(a.shape[1]):
        if k != drop:
            acc = fma_step(acc, a[:, k, None], b[None, :, k])
    return acc


def dot_pairwise4(a, b):
    """fmaf chains over groups of four k, the group sums then added pairwise in f32."""
    parts = []
    for k0 in range(0, a.shape[1], 4):
        acc = np.zeros((len(a), len(b)), F)
        for k in range(k0, k0 + 4):
            acc = fma_step(acc, a[:, k, None], b[None, :, k])
        parts.append(acc)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        assert all(p.dtype == F for p in parts)
    return parts[0]


def epilogue(acc, scale, bias):
    """fmaf(acc, scale, bias) of f32 values through float64 (as fma_step)."""
    return (acc.astype(np.float64) * np.float64(F(scale)) + np.float64(F(bias))).astype(F)


# ---- 3. softmax and sigmoid on the kernels' own logits ---------------------------------------------------
ROWS_KERNEL_SHAPES = [(1, 200), (3, 1), (4, 63), (5, 64), (9, 65), (9, 200), (1, 1)]  # (ni, nt), axis 1
COLS_KERNEL_SHAPES = [(1, 257), (2, 255), (70, 256), (70, 257), (2, 1), (70, 1), (1, 1)]  # (ni, nt), axis 0
SOFTMAX_SCALES = [100.0, 1.0]
SIGMOID_BOUND = HI * (UE + 2 * U)


def softmax_oracle(L, axis):
    """float64 max-subtracted softmax of f32 logits along `axis` -> (p [ni][nt], R, n): R the largest
    max - logit over the reduced axis, n its length.  A NaN or +inf logit makes its row (column) NaN."""
    L = np.asarray(L, F)
    if axis == 1:
        p, _, _, R = softmax_rows_oracle(L)
        return p, R, L.shape[1]
    p, _, _, R = softmax_rows_oracle(np.ascontiguousarray(L.T))
    return np.ascontiguousarray(p.T), R, L.shape[0]


def check_softmax(got, L, axis, what=""):
    """Holds device probabilities to bound_matrix(n, R) of the float64 softmax of the device's logits L."""
    p, R, n = softmax_oracle(L, axis)
    B = bound_matrix(n, R)
    assert got.dtype == F and got.shape == p.shape, what
    nan = np.isnan(p)
    assert np.array_equal(np.isnan(got), nan), what
    err = np.abs(got.astype(np.float64) - p)
    ok = nan | (err <= B * p + TINY)
    assert ok.all(), (what, float(np.nanmax(err / np.maximum(p, TINY))), B)
    live = ~nan.any(axis=axis)
    sums = np.where(nan, 0.0, got.astype(np.float64)).sum(axis=axis)
    assert (np.abs(sums[live] - 1.0) <= n * U).all(), (what, float(np.abs(sums[live] - 1.0).max()), n * U)
    return B


def sigmoid64(L):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(L, np.float64)))


def check_sigmoid(got, L, what=""):
    ref = sigmoid64(L)
    assert got.dtype == F and got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= SIGMOID_BOUND * ref + TINY).all(), (what, float((err / np.maximum(ref, TINY)).max()))


def pattern_case(ni, nt, axis):
    """Integer inputs whose logits at scale -128 are 0 where Z and -128 elsewhere: img = the first ni rows
    of the identity [ni][E], txt[j][i] = 1 - Z[i][j].  Z [ni][nt] is seeded, with (along the softmax axis)
    line 0 holding a single zero logit and line 1 none at all (all equal), where the shape has them.
    -> (img, txt, L), L the f32 logits."""
    rng = np.random.default_rng([ni, nt, axis, 31])
    Z = rng.random((ni, nt)) < 0.3
    Zt = Z if axis == 1 else Z.T  # lines of the softmax as rows
    Zt[0] = False
    Zt[0, (3 * Zt.shape[1]) // 4] = True
    if len(Zt) > 1:
        Zt[1] = False
    E = -(-ni // TK) * TK
    a = np.eye(ni, E, dtype=F)
    b = np.zeros((nt, E), F)
    b[:, :ni] = 1 - Z.T
    L = np.where(Z, F(0), F(-128)).astype(F)
    return a, b, L


PATTERN_SCALE = -128.0
PATTERN_SHAPES = [(9, 200, 1), (5, 65, 1), (70, 257, 0), (2, 255, 0)]  # (ni, nt, axis)


def exact_softmax(L, axis):
    """The f32 softmax of logits that are 0 or -128 along `axis`, bit for bit: expf(l - m) is exactly 1 at
    the maximum and exactly 0 at 128 below it, the sum an exact count c, the probability f32(1) / f32(c)."""
    L = np.asarray(L, F)
    assert np.isin(L, (0.0, -128.0)).all()
    e = (L == L.max(axis=axis, keepdims=True)).astype(F)
    c = e.sum(axis=axis, keepdims=True, dtype=F)
    p = e / c
    assert p.dtype == F
    return p


def saturation_case():
    """E = 16, scale 128, bias 0: dots 0, 1, -1 give logits 0, 128, -128, whose sigmoids are exactly 0.5,
    1.0 (expf(-128) = 0) and 0.0 (expf(128) = inf).  -> (img [3][16], txt [66][16], expected [3][66])."""
    a = np.zeros((3, 16), F)
    a[0, 0], a[1, 1], a[2, 1] = 1, 1, -1
    b = np.zeros((66, 16), F)
    b[:, 1] = 1
    b[::5, 1] = 0  # both rows 1 and 2 see a zero dot there
    d = int_dot(a, b)
    want = np.select([d == 0, d == 1, d == -1], [F(0.5), F(1.0), F(0.0)]).astype(F)
    return a, b, want
