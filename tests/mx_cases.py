"""Cases and checks of the tests of everything that *produces* MX-fp8 bytes (tests/test_gpu_mx_quant.py:
LayerNorm with MX output, the MX GEMM's quantizing epilogue EPI_STOREQ) and of how the MX GEMM is launched at
engine sizes (the persistent tile walk, the row chunks, the pitches).  No GPU import:
tests/test_cpu_mx_cases.py checks all of it on the CPU.

Method.  An MX row is decided by the f32 values the kernel quantizes: scale byte = mx_exp(block amax) + 127,
code = round-to-nearest-even e4m3 of value * 2^-e (oracle/mx_ref.py, pinned to the hardware conversion).
  * Where the f32 values are known exactly (EPI_STOREQ without activation on storeq_case's operands: every
    product, partial sum and the bias add are exact in f32 in any order) the bytes are compared with ==.
  * Where they are known to within a derived per-element delta (LayerNorm: rowwise_cases.f32bound;
    EPI_STOREQ with an activation: act_delta), check_mx holds EVERY scale byte and EVERY code to the
    interval that delta allows: mx_exp and the e4m3 rounding are monotone, so a value in
    [ref - delta, ref + delta] can only give a scale / code between those of the two ends.  There is no
    share of mismatches to tolerate.  What delta costs is ambiguity of the inputs (a block whose two ends
    give different exponents, an element whose two ends give different codes), measured from the reference
    alone and capped (LN_CAPS, ACT_CAPS): an ambiguous element is checked less sharply, so there must be few.
"""
import functools

import numpy as np

from oracle import clip_ref, mx_ref
from tests import gemm_cases as gc
from tests import rowwise_cases as rc

DEC = mx_ref.e4m3_decode_table()
U = 2.0 ** -24  # one f32 rounding, relative
ACTS = {0: None, 1: "quick_gelu", 2: "gelu", 3: "gelu_tanh"}  # common.hpp Act

LN_CAPS = (0.01, 0.005)   # (blocks, elements) ambiguous at most, LayerNorm cases
ACT_CAPS = (0.01, 0.01)   # EPI_STOREQ with an activation


# ---- the oracle's encoder, fast -------------------------------------------------------------------------
def e4m3_encode(y):
    """mx_ref.e4m3_encode (round to nearest even, saturating at 448) from the f32 bits: the walk shape has 17 M
    elements.  tests/test_cpu_mx_cases.py holds it to the oracle's on every code, midpoint and their f32
    neighbours."""
    y = np.ascontiguousarray(y, np.float32)
    u = y.view(np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    r = (a + np.uint32(0x7FFFF) + ((a >> np.uint32(20)) & np.uint32(1))) >> np.uint32(20)  # 3 mantissa bits, RNE
    normal = r.astype(np.int32) - np.int32((127 - 7) << 3)  # rebias 127 -> 7: the e4m3 code of a normal value
    with np.errstate(invalid="ignore", over="ignore"):
        small = np.rint(np.abs(y) * np.float32(512.0)).astype(np.int32)  # below 2^-6: multiples of 2^-9 (8 = 2^-6)
    code = np.where(a < np.uint32(0x3C800000), small, np.minimum(normal, 126))  # 0x3C800000 = 2^-6
    code = np.where(a > np.uint32(0x7F800000), 127, code)  # NaN
    return (code.astype(np.uint8) | (u >> np.uint32(24)).astype(np.uint8) & np.uint8(0x80)).astype(np.uint8)


def quantize_rows(x):
    """mx_ref.quantize_rows with the encoder above."""
    x = np.asarray(x, np.float32)
    xb = _blocks(x)
    e = mx_ref.mx_exp(np.abs(xb).max(-1))
    inv = np.ldexp(np.float32(1.0), -e).astype(np.float32)
    return e4m3_encode(xb * inv[..., None]).reshape(x.shape), (e + 127).astype(np.uint8)


# ---- the interval check ------------------------------------------------------------------------------
def _blocks(a):
    R, C = a.shape
    assert C % 32 == 0
    return a.reshape(R, C // 32, 32)


def scale_range(ref, delta):
    """Allowed block exponents (e_lo, e_hi), [R][C/32]: the block's f32 amax lies between the two ends below,
    and rounding them to f32 keeps the order (rounding is monotone and the amax is an f32)."""
    a = np.abs(ref)
    lo = _blocks(np.maximum(a - delta, 0.0)).max(-1)
    hi = _blocks(a + delta).max(-1)
    e_lo, e_hi = mx_ref.mx_exp(lo.astype(np.float32)), mx_ref.mx_exp(hi.astype(np.float32))
    assert np.all(e_hi - e_lo >= 0) and np.all(e_hi - e_lo <= 1), "delta spans more than two exponents"
    return e_lo, e_hi


def code_range(ref, delta, e):
    """Decoded e4m3 values (lo, hi), [R][C], of the two ends under the block exponents e [R][C/32]."""
    inv = np.ldexp(1.0, -e).repeat(32, -1)
    with np.errstate(over="ignore"):
        lo = DEC[e4m3_encode(((ref - delta) * inv).astype(np.float32))]
        hi = DEC[e4m3_encode(((ref + delta) * inv).astype(np.float32))]
    return lo, hi


def _full(ref, delta):
    ref = np.asarray(ref, np.float64)
    delta = np.broadcast_to(np.asarray(delta, np.float64), ref.shape)
    assert np.all(delta >= 0)
    return ref, delta


def ambiguity(ref, delta):
    """(share of blocks with two allowed exponents, share of elements with two or more allowed codes), from
    the reference alone (codes under the smaller allowed exponent)."""
    ref, delta = _full(ref, delta)
    e_lo, e_hi = scale_range(ref, delta)
    lo, hi = code_range(ref, delta, e_lo)
    return float((e_lo != e_hi).mean()), float((lo != hi).mean())


def check_mx(q, qs, ref, delta, what):
    """MX bytes q [R][C], qs [R][C/32] against fp64 `ref` known to within `delta` (per element, >= 0): every
    scale byte within the allowed exponents, every code, under the scale that was written, within the codes
    of the two ends (compared as decoded values, so -0 equals +0; a NaN code never passes).  Returns
    ambiguity(ref, delta)."""
    ref, delta = _full(ref, delta)
    assert q.shape == ref.shape and qs.shape == (ref.shape[0], ref.shape[1] // 32), (q.shape, qs.shape, ref.shape)
    e_lo, e_hi = scale_range(ref, delta)
    e = qs.astype(np.int64) - 127
    bad_s = (e < e_lo) | (e > e_hi)
    lo, hi = code_range(ref, delta, e)
    got = DEC[q]
    bad_q = ~((got >= lo) & (got <= hi))
    if bad_s.any() or bad_q.any():
        msg = f"{what}: {int(bad_s.sum())} of {bad_s.size} scales and {int(bad_q.sum())} of {bad_q.size} codes out of range"
        if bad_s.any():
            r, c = np.argwhere(bad_s)[0]
            msg += (f"; first scale at [{r}][{c}]: got {int(qs[r, c])}, allowed {int(e_lo[r, c]) + 127}.."
                    f"{int(e_hi[r, c]) + 127}; rows {np.unique(np.argwhere(bad_s)[:, 0])[:8]}, blocks "
                    f"{np.unique(np.argwhere(bad_s)[:, 1])[:8]}")
        if bad_q.any():
            r, c = np.argwhere(bad_q)[0]
            msg += (f"; first code at [{r}][{c}]: got {int(q[r, c]):#04x} = {got[r, c]!r}, allowed {lo[r, c]!r}.."
                    f"{hi[r, c]!r} (ref {ref[r, c]!r} +- {delta[r, c]:.3g}, scale byte {int(qs[r, c // 32])}); rows "
                    f"{np.unique(np.argwhere(bad_q)[:, 0])[:8]}, columns {np.unique(np.argwhere(bad_q)[:, 1])[:8]}")
        raise AssertionError(msg)
    if np.array_equal(e, e_lo):  # (the usual case: the code ranges above are ambiguity()'s)
        return float((e_lo != e_hi).mean()), float((lo != hi).mean())
    return ambiguity(ref, delta)


def assert_bytes(got, want, what):
    """np.array_equal on uint8 arrays, reporting as test_gpu_gemm.assert_same does."""
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {want.size} bytes differ, first at [{r}][{c}]: got "
                             f"{int(got[r, c]):#04x}, want {int(want[r, c]):#04x}; rows {np.unique(bad[:, 0])[:8]}, "
                             f"columns {np.unique(bad[:, 1])[:8]}")


# ---- LayerNorm with MX output --------------------------------------------------------------------------
LN_ROWS = 37
LN_DIMS = [32, 128, 1024, 1152, 1280]  # one block, and every NV (float4 per lane) with D % 32 == 0


class LnMxCase:
    """37 residual-stream-like rows (rowwise_cases.stream_rows: not ln_rows_input, whose |mean| = 100 std and
    constant rows make f32bound wide and 17 % of the elements ambiguous) on the f32 or the f16 stream; ref =
    fp64 LayerNorm of the stored row, delta = rowwise_cases.f32bound (64 roundings of the f32 LayerNorm)."""

    def __init__(self, D, x16):
        self.D, self.x16 = D, x16
        self.x = rc.stream(rc.stream_rows(LN_ROWS, D, D + x16), x16)
        self.w, self.b = rc.ln_params(D, D)
        self.ref, self.delta = ln_ref_delta(self.x, self.w, self.b)


def ln_ref_delta(x, w, b):
    ref, _, rstd = rc.ln_ref(x, w, b)
    return ref, rc.f32bound(ref, x, w, b, rstd)


@functools.lru_cache(maxsize=None)
def ln_case(D, x16):
    return LnMxCase(D, x16)


# ---- EPI_STOREQ: exact operands ------------------------------------------------------------------------
STOREQ_SHAPES = [(300, 160, 256),  # M and N tails on both tiles
                 (77, 64, 128),    # one K step
                 (33, 160, 128),   # one row past a 32-row MFMA group
                 (5, 96, 256), (1, 128, 128)]  # the pruned last layer's M = B
CHUNK_SHAPE = (700, 160, 256)  # the row-chunk test: 256 + 256 + 188 rows under a cap of 256

_POS = DEC[:127]


def on_midpoint(x):
    """x (fp64 magnitudes below 448) exactly between two e4m3 values: an odd multiple of half the spacing,
    2^-10 below 2^-6, else 2^(E - 4) for x in [2^E, 2^(E + 1))."""
    m, _ = np.frexp(x)
    k = np.where(x < 2.0 ** -6, x * 1024.0, m * 32.0)
    return (k == np.rint(k)) & (np.rint(k) % 2 == 1) & (x < 448.0)


class StoreqCase:
    """Operands of the quantizing epilogue whose pre-activation t = A.W^T + bias is exact in f32 in any order.
    A: integers in [-4, 4]; W: integers in [-4, 4] times 2^-6, the rows of column block j (32 output columns)
    times 2^(j mod 5 - 2); every 32-block of A and W holds a +-4, so both are exact in MX-fp8.  bias:
    multiples of 2^-6 in [-2, 2].  One column block (`zero`) has W rows 0 and bias 0: scale byte 0, codes 0."""

    def __init__(self, M, N, K, seed=0):
        rng = np.random.default_rng([M, N, K, seed, 2])
        self.M, self.N, self.K, self.seed = M, N, K, seed
        nb = N // 32
        self.zero = 0  # (the first block: a 2-block row keeps its livelier second one, scaled by 2^-1)
        A, Wi = gc.ints(rng, (M, K)), gc.ints(rng, (N, K))
        for X in (A, Wi):
            blocks = X.reshape(X.shape[0], K // 32, 32)
            at = rng.integers(0, 32, size=blocks.shape[:2])
            np.put_along_axis(blocks, at[..., None], rng.choice([-4.0, 4.0], size=blocks.shape[:2])[..., None], -1)
        bi = rng.integers(-128, 129, size=N)
        Wi[32 * self.zero:32 * self.zero + 32] = 0
        bi[32 * self.zero:32 * self.zero + 32] = 0
        self.cexp = (np.arange(nb) % 5 - 2).repeat(32)  # per output column: W row n is scaled by 2^cexp[n]
        self.A = A
        self.W = (Wi * np.exp2(self.cexp - 6.0)[:, None]).astype(np.float32)
        self.bias = (bi * 2.0 ** -6).astype(np.float32)
        self.aq, self.as_ = mx_ref.quantize_rows(self.A)
        self.wq, self.ws = mx_ref.quantize_rows(self.W)
        for X, q, s in ((self.A, self.aq, self.as_), (self.W, self.wq, self.ws)):
            assert np.array_equal(mx_ref.dequantize(q, s), X)
        self.ops = (self.aq, self.as_, self.wq, self.ws)
        # t in fp64: integers times 2^(cexp - 6) plus multiples of 2^-6, far below 2^24 units (exact_sum_bound)
        self.t = gc.acc_of(A, Wi) * np.exp2(self.cexp - 6.0)[None, :] + self.bias.astype(np.float64)[None, :]
        self.t32 = self.t.astype(np.float32)
        assert np.array_equal(self.t32, self.t)
        self.rq, self.rs = quantize_rows(self.t32)  # act 0: the bytes, exactly
        p = self.props = self.properties()
        assert p["scales"] >= 4, p
        assert np.all(self.rs[:, self.zero] == 0) and np.all(self.rq[:, 32 * self.zero:32 * self.zero + 32] == 0)
        assert p["max_in_first_half"] >= 0.2 and p["max_in_second_half"] >= 0.2, p
        assert p["midpoints"] >= 0.01, p

    def properties(self):
        a = _blocks(np.abs(self.t))
        first, second = a[..., :16].max(-1), a[..., 16:].max(-1)  # the two lanes of the xmax32 exchange
        x = np.abs(self.t) * np.ldexp(1.0, 127 - self.rs.astype(np.int64)).repeat(32, -1)
        return dict(scales=len(np.unique(self.rs)), max_in_first_half=float((first > second).mean()),
                    max_in_second_half=float((second > first).mean()),
                    midpoints=float(on_midpoint(x).mean()),  # exactly between two codes: nearest-EVEN decides
                    t_min=float(self.t.min()), t_max=float(self.t.max()), t_std=float(self.t.std()))

    def z(self, act):
        """fp64 act(t)."""
        return act_ref64(act, self.t)

    def delta(self, act):
        return np.zeros_like(self.t) if act == 0 else act_delta(act, self.t, self.z(act))


@functools.lru_cache(maxsize=None)
def storeq_case(M, N, K):
    """The first seed whose case meets the constructor's assertions (small cases: four distinct scales in a
    handful of blocks are not a given)."""
    err = None
    for seed in range(64):
        try:
            return StoreqCase(M, N, K, seed)
        except AssertionError as e:
            err = e
    raise err


def exact_sum_bound(K):
    """The largest partial sum of t, in units of its smallest term, over the column-block scalings: products
    are integers (<= 16) times 2^(s - 6), s in [-2, 2], the bias is an integer (<= 128) times 2^-6."""
    worst = 0
    for s in range(-2, 3):
        unit = 2.0 ** (min(s, 0) - 6)
        worst = max(worst, (16 * K * 2.0 ** (s - 6) + 128 * 2.0 ** -6) / unit)
    return worst


# ---- the activations' error (common.hpp apply_act) on an exact f32 t -------------------------------------
# v_exp_f32 / v_rcp_f32: 1 ulp = 2 u each is an assumption (no published figure used), taken times 4: T = 8 u


def act_ref64(act, t):
    """fp64 act(t) as clip_ref.act_fn defines it, in the forms that keep their relative accuracy in the
    negative tail (1 + erf and 1 + tanh cancel there): 0.5 t erfc(-t / sqrt 2), and t sigmoid(2 u) for
    0.5 t (1 + tanh u), an identity.  tests/test_cpu_mx_cases.py holds them to clip_ref.act_fn."""
    t = np.asarray(t, np.float64)
    if act == 0:
        return t
    if act == 1:
        return clip_ref.act_fn("quick_gelu", t)
    if act == 2:
        from scipy.special import erfc
        return 0.5 * t * erfc(-t / np.sqrt(2.0))
    if act == 3:
        with np.errstate(over="ignore"):
            return t / (1.0 + np.exp(-2.0 * np.sqrt(2.0 / np.pi) * (t + 0.044715 * t ** 3)))
    raise ValueError(act)


def act_delta(act, t, z):
    """|apply_act<act>(t) - z| allowed, z = fp64 act(t), t an exact f32.  Derivation: DESIGN.md (MX-fp8 tests);
    u = 2^-24 per f32 operation or rounded constant, T = 8 u per hardware transcendental, first order.
      QuickGELU  t * rcp(1 + exp2(fl(t c))), c = -1.702 log2 e:
                 exponent |t c| (2 u) -> exp2 relative ln 2 * 2.4555 |t| * 2 u + T <= 3.5 |t| u + T; the
                 sigmoid depends on it with sensitivity <= 1; + u (1 + E) + T (rcp) + u (product):
                 (18 + 3.5 |t|) u |z|
      tanh-GELU  t * rcp(1 + exp2(fl(-zz log2 e))), zz = fl(2 k0 fma(k1 t, t t, t)), w = |t| (1 + k1 t^2):
                 zz relative 7 u, times log2 e 2 u; exponent magnitude 2.3023 w -> exp2 relative
                 ln 2 * 2.3023 w * 9 u + T <= 14.5 w u + T; the rest as above:  (18 + 14.5 w) u |z|
    Both plus (1 + |t|) 2^-126: past |t| of about 12 the exponential overflows or the quotient leaves the
    normal f32 range (flushed to zero), where a relative bound on |z| < 2^-126 |t| means nothing.
      erf-GELU   fl(0.5 t * fl(1 + erf_f(s))), s = fl(t / sqrt 2), erf_f = 1 - Q, Q = P(r) E, r = rcp(1 + p |s|),
                 E = exp(-s^2) <= 1:  2 u |z| + 0.5 |t| d_erf,
                 d_erf = 1.5e-7 (Abramowitz-Stegun 7.1.26, fast_erf's comment) + u (the rounding of 1 - Q)
                         + (55 + 2.3 |s| + 3 s^2) u E
                 (in units of u E: 35 r's 10 u through P, |sum k a_k r^k| <= 3.5 on (0, 1]; 4.5 the rounded
                 coefficients; 6 the Horner steps and P's last product; 3 s^2 + 8 the exponential's argument
                 and v_exp; 1 the product with E; 2.3 |s| the two roundings of s through erf')
    """
    t, z = np.asarray(t, np.float64), np.asarray(z, np.float64)
    a = np.abs(t)
    tiny = np.where(a > 0, (1 + a) * 2.0 ** -126, 0.0)  # (t = 0 gives 0 exactly in every form)
    if act == 1:
        return (18 + 3.5 * a) * U * np.abs(z) + tiny
    if act == 3:
        return (18 + 14.5 * a * (1 + 0.044715 * a * a)) * U * np.abs(z) + tiny
    if act == 2:
        s2 = a * a / 2
        return 2 * U * np.abs(z) + 0.5 * a * (1.5e-7 + U + (55 + 2.3 * np.sqrt(s2) + 3 * s2) * U * np.exp(-s2))
    raise ValueError(act)


def _fma(a, b, c):
    """f32 fma: the product of two f32 is exact in fp64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def act_emulate_f32(act, t):
    """apply_act<act> restated in numpy f32 (numpy's exp2 and divide for v_exp_f32 and v_rcp_f32)."""
    f = np.float32
    x = np.asarray(t, f)
    if act == 1:
        return x * (f(1) / (f(1) + np.exp2(x * f(-2.4554669596))))
    if act == 3:
        k0, k1 = f(0.7978845608028654), f(0.044715)
        zz = (f(2.0) * k0) * _fma(k1 * x, x * x, x)
        with np.errstate(over="ignore"):
            return x * (f(1) / (f(1) + np.exp2(-zz * f(1.4426950408889634))))
    if act == 2:
        s = x * f(0.70710678118654752)
        ax = np.abs(s)
        r = f(1) / _fma(f(0.3275911), ax, f(1))
        p = _fma(f(1.061405429), r, f(-1.453152027))
        for c in (1.421413741, -0.284496736, 0.254829592):
            p = _fma(p, r, f(c))
        y = f(1) - p * r * np.exp2((-ax * ax) * f(1.4426950408889634))
        out = f(0.5) * x * (f(1) + np.copysign(y, s))
        assert out.dtype == f
        return out
    raise ValueError(act)


# ---- the persistent walk ---------------------------------------------------------------------------------
WALK_N, WALK_K = 33 * 128 - 96, 256  # 33 column tiles, an N tail of 32
MX_TILE_DIMS = {2: (256, 1), 3: (128, 2)}  # MxTile id -> (BM, resident blocks per CU); BN = 128


def walk_shape(cus):
    """The smallest M = 128 r + 104 with more than 4 cus tiles of 128x128 (two resident rounds of the
    128x128 tile, so some block takes a third tile and reuses its first bias slice)."""
    r = -(-(4 * cus + 1) // 33) - 1
    return 128 * r + 104, WALK_N, WALK_K


def walk_tiles_per_block(M, N, tile, cus):
    """Tiles each block of gemm_mx_kernel walks (its XCD-aware split), as launch_mx_cfg sizes the grid."""
    BM, per_cu = MX_TILE_DIMS[tile]
    ntiles = -(-M // BM) * -(-N // 128)
    nb = min(ntiles, cus * per_cu)
    if nb % 8 or nb >= ntiles:
        return [1] * nb
    q, r = divmod(ntiles, 8)
    counts = []
    for b in range(nb):
        x = b & 7
        start = x * (q + 1) if x < r else r * (q + 1) + (x - r) * q
        first, end = start + (b >> 3), start + q + (1 if x < r else 0)
        counts.append(max(0, -(-(end - first) // (nb >> 3))))
    assert sum(counts) == ntiles
    return counts


# ---- mutants (tests/test_cpu_mx_cases.py: each must be rejected) -------------------------------------------
def requantize(x32, e):
    """Codes of f32 x under given block exponents e [R][C/32]."""
    inv = np.ldexp(np.float32(1.0), -e).astype(np.float32).repeat(32, -1)
    with np.errstate(over="ignore"):
        return mx_ref.e4m3_encode(x32 * inv)


def mutant_scale_plus_one(x32, r, c):
    """Block [r][c]'s scale one too large, its codes quantized under it (a floating format hides it)."""
    q, s = mx_ref.quantize_rows(x32)
    e = s.astype(np.int64) - 127
    e[r, c] += 1
    return requantize(x32, e), (e + 127).astype(np.uint8)


def mutant_amax_of_16(x32):
    """The lane-pair exchange missing: each 16-column half quantized under its own amax, the scale byte the
    first half's."""
    R, C = x32.shape
    e16 = mx_ref.mx_exp(np.abs(x32).reshape(R, C // 16, 16).max(-1))
    inv = np.ldexp(np.float32(1.0), -e16).astype(np.float32).repeat(16, -1)
    return mx_ref.e4m3_encode(x32 * inv), (e16[:, ::2] + 127).astype(np.uint8)


def mutant_truncate(x32):
    """Codes truncated toward zero instead of rounded to nearest even."""
    q, s = mx_ref.quantize_rows(x32)
    y = np.abs(_blocks(x32) * np.ldexp(np.float32(1.0), 127 - s.astype(np.int64)).astype(np.float32)[..., None])
    code = np.clip(np.searchsorted(_POS, y.astype(np.float64), side="right") - 1, 0, 126)
    return (code.reshape(x32.shape) | (q & 0x80)).astype(np.uint8), s


def mutant_neighbour_bias(c):
    """EPI_STOREQ with the bias slice of the neighbouring 128-column tile."""
    n = (np.arange(c.N) + 128) % c.N
    t = (c.t - c.bias.astype(np.float64)[None, :] + c.bias.astype(np.float64)[None, n]).astype(np.float32)
    return mx_ref.quantize_rows(t)


def mutant_partner_amax(c):
    """The last row under the block amax of another row (the nearest one above it whose scales differ; at
    M = 1 its own, one block over): its scale bytes are that row's, its codes quantized under them."""
    q, s = mx_ref.quantize_rows(c.t32)
    e = s.astype(np.int64) - 127
    other = [r for r in range(c.M - 2, -1, -1) if np.any(e[r] != e[-1])]
    e[-1] = e[other[0]] if other else np.roll(e[-1], 1)
    return requantize(c.t32, e), (e + 127).astype(np.uint8)
