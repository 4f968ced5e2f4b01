"""Inputs and exact references of the GEMM tests (tests/test_gpu_gemm.py), checked without a GPU by
tests/test_cpu_gemm_cases.py.

Method: integer-exact operands.  A and W hold integers in [-4, 4] (exact in bf16 and f16), so every
product and every partial sum of a GEMM is an integer of magnitude <= 16 K, far below 2^24: the f32
accumulator of the MFMA chain is exact in any summation order, for any tile, split or schedule.  What
follows the accumulator is a short, fixed sequence of IEEE f32 operations (kernels.hpp Epi):
    v = f32(acc) + bias[n];   v = v + x;   out = round_T(v)
(x = the residual element, or the positional-embedding element of the patch epilogue; round_T = one
rounding to bf16 / f16, or none for f32 outputs).  numpy's f32 adds and its f16 conversion round to
nearest even as the hardware does, so the reference below reproduces the kernels bit for bit and the
GPU tests compare with ==: one wrong element, row, column, dropped K-step, missed tile or extra
rounding fails.  fp64 stands behind the reference (ref64): the f32 sequence is within one rounding per
add, plus the output rounding, of it.

bias, resid and pos are arbitrary f32 (all mantissa bits in use) so that each add and the final rounding
are exercised; their spread (tens) is wide beside a 16-bit ulp of the results (|v| < 2^11: at most 8 in
bf16, 1 in f16), so that a wrong bias column, residual row or positional row changes the bits.
"""
import functools

import numpy as np

from tests.rowwise_cases import BF16, F16, rel16, round16

TILES = [2, 3, 13, 14, 15, 17, 18, 26]  # kernels.hpp kGemmTiles (the pipelined tiles)
TILE_IDS = ["pipe256x128", "pipe256x256", "w8_192x256", "rs_256x256", "rs_160x128", "rs_w8_160x128",
            "half_256x256", "w8_224x192"]
SKINNY, GENERAL = 100, 101
SHAPES = [(700, 520, 128), (333, 136, 192), (77, 64, 256), (1, 16, 128)]
GENERAL_SHAPES = [(333, 100, 192), (333, 136, 64)]  # mode 0 only: a 16-bit row of 100, one K-step
WALK_SHAPE = (8300, 2056, 128)  # more tiles than resident blocks, for every tile
WALK_MODE, WALK_TYPE = 3, BF16  # as the engines' default c_proj: the f16 residual stream
PITCH_SHAPE = (333, 136, 192)
PAD_A, PAD_W, PAD_O = 8, 24, 8
SENTINEL = np.float32(24576.0)  # 1.5 * 2^14: exact in bf16, f16 and f32, and beyond every result (|v| < 2^11)
MODES = [0, 1, 2, 3]  # clipgpu_test_gemm: 0 store16, 1 residual f32, 2 store32, 3 residual f16 stream


def skinny_applies(M, N, K):
    """gemm.hip skinny_ok at dense pitches."""
    return M <= 256 and N % 16 == 0 and K % 256 == 0


def tiles_for(M, N, K):
    return TILES + [GENERAL] + ([SKINNY] if skinny_applies(M, N, K) else [])


def ints(rng, shape):
    return rng.integers(-4, 5, size=shape).astype(np.float32)


def spread(rng, shape, scale):
    """Arbitrary f32 values of spread `scale`: every mantissa bit in use."""
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def distinct_vec(rng, n, scale):
    """n distinct non-zero f32 values."""
    while True:
        v = spread(rng, n, scale)
        if len(np.unique(v)) == n and np.all(v != 0):
            return v


def distinct_rows(rng, rows, cols, scale):
    while True:
        v = spread(rng, (rows, cols), scale)
        if len(np.unique(v, axis=0)) == rows:
            return v


class GemmCase:
    """A [M][K], W [N][K] integers; bias [N]; resid [M][N] (f32; resid16 = as the f16 stream stores it)."""

    def __init__(self, M, N, K, seed=0):
        rng = np.random.default_rng([M, N, K, seed])
        self.M, self.N, self.K = M, N, K
        self.A, self.W = ints(rng, (M, K)), ints(rng, (N, K))
        self.bias = distinct_vec(rng, N, 40.0)
        self.resid = spread(rng, (M, N), 30.0)
        self.resid16 = self.resid.astype(np.float16).astype(np.float32)

    def x(self, mode):
        """The residual the hook is given for `mode` (None for the store epilogues)."""
        return self.resid if mode == 1 else self.resid16 if mode == 3 else None

    def ref(self, mode, dtype, bias=True, A=None, W=None, x=None):
        A = self.A if A is None else A
        W = self.W if W is None else W
        x = self.x(mode) if x is None else x
        return epilogue(acc_of(A, W), self.bias if bias else None, x, out_type(mode, dtype))

    def ref64(self, mode, bias=True):
        r = acc_of(self.A, self.W).astype(np.float64)
        if bias:
            r = r + self.bias.astype(np.float64)
        x = self.x(mode)
        return r if x is None else r + x.astype(np.float64)


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, seed=0):
    return GemmCase(M, N, K, seed)


def acc_of(A, W):
    """int64 A . W^T of integer-valued matrices.  (Through the fp64 BLAS: every product and partial sum is
    an integer far below 2^53, so the fp64 product is exact in any order; checked against rint.)"""
    p = np.asarray(A, np.float64) @ np.asarray(W, np.float64).T
    acc = np.rint(p).astype(np.int64)
    assert np.array_equal(acc, p)
    return acc


def out_type(mode, dtype):
    """What the epilogue rounds to: 'f32', or a 16-bit type id."""
    return dtype if mode == 0 else "f32" if mode in (1, 2) else F16


def round_out(v, ot):
    assert v.dtype == np.float32
    return v if ot == "f32" else round16(v, ot)


def epilogue(acc, bias, x, ot):
    """The kernels' epilogue in numpy f32, in their order: (f32(acc) + bias) + x, then one rounding."""
    v = acc.astype(np.float32)
    assert np.array_equal(v.astype(np.int64), acc)  # |acc| < 2^24
    if bias is not None:
        v = v + np.asarray(bias, np.float32)[None, :]
    if x is not None:
        v = v + np.asarray(x, np.float32)
    assert v.dtype == np.float32
    return round_out(v, ot)


def shuffled_block_acc(A, W, seed):
    """The accumulator as an f32 chain over 32-wide K blocks taken in a shuffled order (what a different
    tile, split or schedule would do): exact inputs make it order-independent."""
    K = A.shape[1]
    order = np.random.default_rng(seed).permutation(K // 32)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for b in order:
        part = (A[:, 32 * b:32 * b + 32].astype(np.float64) @ W[:, 32 * b:32 * b + 32].astype(np.float64).T)
        acc = acc + part.astype(np.float32)
    assert acc.dtype == np.float32
    return acc


def padded(a, ld, fill):
    """[rows][ld] with a in the leading columns and `fill` in the pad columns."""
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, :a.shape[1]] = a
    return out


# ---- the two-roundings case ---------------------------------------------------------------------
# A bf16 result rounded through f16 first (result -> f16 -> bf16) differs from the single rounding only
# where the f16 value lands on a bf16 tie.  This case puts (almost) every element there: W even, so acc is
# even; |acc| in [128, 256) for nearly all elements (bf16 ulp 1, f16 ulp 1/8); bias = 0.5 + e with
# 0 < e < 1/16: f16 rounds acc + 0.5 + e to the tie acc + 0.5, whose even bf16 neighbour is acc, while the
# single rounding gives acc + 1.  K = 128 with A's second half zero (a pipelined tile needs two K-steps).
@functools.lru_cache(maxsize=None)
def rounding_case(M=333, N=136):
    c = GemmCase.__new__(GemmCase)
    rng = np.random.default_rng([M, N, 77])
    c.M, c.N, c.K = M, N, 128
    c.A = np.zeros((M, 128), np.float32)
    c.A[:, :64] = rng.integers(0, 3, size=(M, 64)) * rng.choice([-1, 1], size=(M, 1))
    c.W = (rng.choice([2, 4], size=(N, 128)) * rng.choice([-1, 1], size=(N, 1))).astype(np.float32)
    c.bias = (0.5 + np.linspace(0.01, 0.05, N)).astype(np.float32)
    c.resid = c.resid16 = None
    return c


# ---- the patch GEMM ------------------------------------------------------------------------------
class PatchCase:
    """rows [B G^2][Kp], W [D][Kp] integers; bias [D]; pos [G^2 + cls][D]; x0 = the stream before the
    launch: the sentinel everywhere (class rows must keep it)."""

    def __init__(self, cls, B, G, Kp, D, seed=0):
        rng = np.random.default_rng([cls, B, G, Kp, D, seed])
        self.cls, self.B, self.G, self.Kp, self.D = cls, B, G, Kp, D
        self.G2, self.tokens = G * G, G * G + cls
        self.rows, self.W = ints(rng, (B * G * G, Kp)), ints(rng, (D, Kp))
        self.bias = distinct_vec(rng, D, 40.0)
        self.pos = distinct_rows(rng, self.tokens, D, 30.0)
        self.x0 = np.full((B * self.tokens, D), SENTINEL, np.float32)

    def ref(self, x16, bias=True, pos_shift=None, row_tokens=None):
        """x after the launch.  pos_shift / row_tokens: the mutants (pos[p] for pos[cls + p]; G^2 for
        G^2 + cls in the token row)."""
        cls, G2 = self.cls, self.G2
        pos_shift = cls if pos_shift is None else pos_shift
        row_tokens = self.tokens if row_tokens is None else row_tokens
        m = np.arange(self.B * G2)
        b, p = m // G2, m % G2
        v = epilogue(acc_of(self.rows, self.W), self.bias if bias else None, self.pos[pos_shift + p],
                     F16 if x16 else "f32")
        out = self.x0.copy()
        out[b * row_tokens + cls + p] = v
        return out

    def ref64(self, bias=True):
        m = np.arange(self.B * self.G2)
        r = acc_of(self.rows, self.W).astype(np.float64) + self.pos[self.cls + m % self.G2].astype(np.float64)
        return r + self.bias.astype(np.float64) if bias else r

    def patch_rows_of(self, out):
        """The patch-token rows of a stream, in patch-row order."""
        m = np.arange(self.B * self.G2)
        return out[m // self.G2 * self.tokens + self.cls + m % self.G2]


@functools.lru_cache(maxsize=None)
def patch_case(cls, B, G, Kp, D):
    return PatchCase(cls, B, G, Kp, D)


PATCH_SHAPES = [(40, 3, 192, 128), (40, 3, 192, 136), (5, 1, 192, 128)]  # (B, G, Kp, D)


# ---- MX-fp8 ----------------------------------------------------------------------------------------
MX_SHAPES = [(300, 160, 256), (77, 64, 128)]
MX_MODES = [0, 1, 2, 4]  # clipgpu_test_gemm_mx: 0 store16, 1 residual f32, 2 store32, 4 residual f16 stream
MX_TILES = [0, 2, 3]


def mx_out_type(mode, dtype):
    return dtype if mode == 0 else F16 if mode == 4 else "f32"


class MxCase(GemmCase):
    """Integer operands whose MX-fp8 form is exact: every 32-block holds a +-4, so every block has the
    scale 2^-6 and the codes are the integers times 64 (all e4m3 values)."""

    def __init__(self, M, N, K, seed=0):
        from oracle import mx_ref
        super().__init__(M, N, K, seed)
        rng = np.random.default_rng([M, N, K, seed, 1])
        for X in (self.A, self.W):
            blocks = X.reshape(X.shape[0], K // 32, 32)
            at = rng.integers(0, 32, size=blocks.shape[:2])
            np.put_along_axis(blocks, at[..., None], rng.choice([-4.0, 4.0], size=blocks.shape[:2])[..., None], -1)
        self.aq, self.as_ = mx_ref.quantize_rows(self.A)
        self.wq, self.ws = mx_ref.quantize_rows(self.W)
        for X, q, s in ((self.A, self.aq, self.as_), (self.W, self.wq, self.ws)):
            assert len(np.unique(s)) == 1  # one scale
            assert np.array_equal(mx_ref.dequantize(q, s), X)

    def x(self, mode):
        return self.resid if mode == 1 else self.resid16 if mode == 4 else None

    def ref(self, mode, dtype, bias=True):
        return epilogue(acc_of(self.A, self.W), self.bias if bias else None, self.x(mode), mx_out_type(mode, dtype))


@functools.lru_cache(maxsize=None)
def mx_case(M, N, K):
    return MxCase(M, N, K)


def mx_random_operands(M, N, K, seed, k_spread=False):
    """Random MX operands (as tests/test_gpu_mx.py); k_spread: A's block scales run over 2^-6 .. 2^6 along
    K, W's over the inverse."""
    from oracle import mx_ref
    rng = np.random.default_rng([M, N, K, seed])
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    if k_spread:
        e = np.resize(np.arange(-6, 7), K // 32)
        A = A * np.exp2(e).repeat(32)[None, :].astype(np.float32)
        W = W * np.exp2(-e).repeat(32)[None, :].astype(np.float32)
    return mx_ref.quantize_rows(A) + mx_ref.quantize_rows(W)


# ---- agreement with fp64 ---------------------------------------------------------------------------
def f64_bound(ref64, terms, ot):
    """|f32-ordered reference - fp64| allowed: 2^-23 relative per add (of a partial result no larger than
    `terms`, the sum of the magnitudes added; two adds), plus one rounding to the output type (rel16)."""
    b = 2 * 2.0 ** -23 * terms
    return b if ot == "f32" else b + rel16(ot) * (np.abs(ref64) + b)
