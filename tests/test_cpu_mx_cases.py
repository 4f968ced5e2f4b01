"""tests/mx_cases.py without a GPU: the interval check passes a correct model and rejects each mutant, the
cases meet their constructor assertions and ambiguity caps, the activation bound holds a numpy-f32 restatement
of common.hpp apply_act, and the walk shape sums exactly.  What tests/test_gpu_mx_quant.py holds the kernels
to is checked here first."""
import numpy as np
import pytest

from oracle import clip_ref, mx_ref
from tests import gemm_cases as gc
from tests import mx_cases as mc
from tests import rowwise_cases as rc

LN_CASES = [(D, x16) for D in mc.LN_DIMS for x16 in (0, 1)]
SHAPES = mc.STOREQ_SHAPES + [mc.CHUNK_SHAPE]
EACH_SHAPE = pytest.mark.parametrize("M,N,K", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
MI355X_CUS = 256


def rejected(q, qs, ref, delta):
    """check_mx's complaint about (q, qs), or None."""
    try:
        mc.check_mx(q, qs, ref, delta, "mutant")
    except AssertionError as e:
        return str(e)
    return None


def counts(msg):
    """(scales, codes) out of range, from check_mx's message."""
    w = msg.split()
    return int(w[1]), int(w[w.index("scales") + 2])


def spread_rows(R, C, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, C)) * np.exp2(rng.integers(-6, 6, (R, C // 32, 1))).repeat(32, -1).reshape(R, C)
            ).astype(np.float32)


# ---- the encoder under the check ---------------------------------------------------------------------------
def test_fast_encoder_is_the_oracles():
    """mx_cases.e4m3_encode == mx_ref.e4m3_encode on every e4m3 value, every midpoint, values past the range,
    the f32 neighbours of all of them, both signs, and random values over 22 binades; on_midpoint marks
    exactly the midpoints."""
    pos = mc.DEC[:127]
    mids = (pos[:-1] + pos[1:]) / 2
    vals = np.concatenate([pos, mids, [448, 464, 480, 1000, 3e38, 2.0 ** -10, 2.0 ** -11, 1e-40]]).astype(np.float32)
    both = np.concatenate([vals, np.nextafter(vals, np.float32(np.inf)), np.nextafter(vals, np.float32(-np.inf))])
    rng = np.random.default_rng(0)
    rand = (rng.standard_normal(200000) * np.exp2(rng.integers(-12, 10, 200000))).astype(np.float32)
    x = np.concatenate([both, -both, rand, [np.inf, -np.inf]]).astype(np.float32)
    assert np.array_equal(mc.e4m3_encode(x), mx_ref.e4m3_encode(x))
    assert mc.e4m3_encode(np.array([np.nan], np.float32))[0] & 0x7F == 0x7F
    m = np.abs(both[both < 448]).astype(np.float64)
    assert np.array_equal(mc.on_midpoint(m), np.isin(m, mids)) and mc.on_midpoint(m).sum() >= 126
    r = spread_rows(64, 256)
    for a, b in zip(mc.quantize_rows(r), mx_ref.quantize_rows(r)):
        assert np.array_equal(a, b)


def test_interval_check_is_equality_at_delta_zero():
    """delta = 0 on exact f32 values: check_mx accepts the oracle's bytes, nothing is ambiguous, and any other
    code or scale byte (one step up or down) is rejected -- except -0 for +0."""
    x = spread_rows(64, 256)
    q, s = mx_ref.quantize_rows(x)
    assert mc.check_mx(q, s, x, 0.0, "oracle") == (0.0, 0.0)
    for step in (1, -1):
        q2 = q.copy()
        q2[5, 7] = np.clip(int(q[5, 7] & 0x7F) + step, 0, 126) | (q[5, 7] & 0x80)
        assert q2[5, 7] != q[5, 7] and counts(rejected(q2, s, x, 0.0)) == (0, 1)
        s2 = s.copy()
        s2[9, 3] = int(s[9, 3]) + step
        assert counts(rejected(q, s2, x, 0.0))[0] == 1
    x[0, :32] = 0.0
    q, s = mx_ref.quantize_rows(x)
    q[0, 3] = 0x80  # -0
    mc.check_mx(q, s, x, 0.0, "-0")
    q[0, 4] = 0x7F  # NaN
    assert counts(rejected(q, s, x, 0.0)) == (0, 1)


# ---- LayerNorm -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,x16", LN_CASES)
def test_ln_cases_pass_a_correct_model_within_the_caps(D, x16):
    """The numpy-f32 LayerNorm (rowwise_cases.ln_emulate_f32), quantized by the oracle, passes check_mx at
    delta = f32bound; the case's ambiguity is under the caps (measured: at most 0.17 % of elements, no block)."""
    c = mc.ln_case(D, x16)
    out, _ = rc.ln_emulate_f32(c.x, c.w, c.b)
    assert np.all(np.abs(out - c.ref) <= c.delta)
    blocks, elements = mc.check_mx(*mx_ref.quantize_rows(out), c.ref, c.delta, f"D {D} x16 {x16}")
    print(f"\n[mx] LN D {D} x16 {x16}: ambiguous blocks {blocks:.4%} elements {elements:.4%}")
    assert (blocks, elements) == mc.ambiguity(c.ref, c.delta)
    assert blocks <= mc.LN_CAPS[0] and elements <= mc.LN_CAPS[1]


@pytest.mark.parametrize("D,x16", LN_CASES)
def test_ln_cases_reject_the_mutants(D, x16):
    c = mc.ln_case(D, x16)
    out, _ = rc.ln_emulate_f32(c.x, c.w, c.b)
    e_lo, e_hi = mc.scale_range(c.ref, c.delta)
    r, b = np.argwhere(e_lo == e_hi)[D // 32 * 17 % (e_lo == e_hi).sum()]  # a block with one allowed exponent
    msg = rejected(*mc.mutant_scale_plus_one(out, r, b), c.ref, c.delta)
    assert msg and counts(msg) == (1, 0), msg  # one scale, and no code: a floating format hides it
    msg = rejected(*mc.mutant_amax_of_16(out), c.ref, c.delta)
    assert msg and counts(msg)[1] >= 0.1 * out.size, msg
    msg = rejected(*mc.mutant_truncate(out), c.ref, c.delta)
    assert msg and counts(msg)[0] == 0 and counts(msg)[1] >= 0.3 * out.size, msg


# ---- EPI_STOREQ ------------------------------------------------------------------------------------------------
@EACH_SHAPE
def test_storeq_cases_and_caps(M, N, K):
    """The constructor's assertions (re-stated), the exactness of t, and the ambiguity caps per activation."""
    c = mc.storeq_case(M, N, K)
    p = c.props
    print(f"\n[mx] storeq {M}x{N}x{K} seed {c.seed}: {p}")
    assert p["scales"] >= 4 and min(p["max_in_first_half"], p["max_in_second_half"]) >= 0.2 and p["midpoints"] >= 0.01
    assert np.array_equal(c.t32, c.t) and mc.exact_sum_bound(K) < 2 ** 24
    # t by another route: the dequantized operands in fp64
    assert np.array_equal(mx_ref.mx_gemm_ref(*c.ops, c.bias), c.t)
    # and as an f32 chain over K blocks in a shuffled order
    acc = gc.shuffled_block_acc(mx_ref.dequantize(c.aq, c.as_), mx_ref.dequantize(c.wq, c.ws), 5)
    assert np.array_equal(acc + c.bias[None, :], c.t32)
    assert mc.check_mx(c.rq, c.rs, c.t, 0.0, "act 0") == (0.0, 0.0)
    for act in (1, 2, 3):
        blocks, elements = mc.ambiguity(c.z(act), c.delta(act))
        print(f"[mx] storeq {M}x{N}x{K} act {act}: ambiguous blocks {blocks:.4%} elements {elements:.4%}")
        assert blocks <= mc.ACT_CAPS[0] and elements <= mc.ACT_CAPS[1]


@EACH_SHAPE
def test_activation_bound_holds_the_f32_forms(M, N, K):
    """apply_act's three forms restated in numpy f32 stay inside act_delta of the fp64 activation, and their
    oracle quantization passes check_mx."""
    c = mc.storeq_case(M, N, K)
    for act in (1, 2, 3):
        z, d = c.z(act), c.delta(act)
        y = mc.act_emulate_f32(act, c.t32)
        err = np.abs(y - z)
        assert np.all(err <= d), (act, float((err / np.maximum(d, 1e-300)).max()))
        mc.check_mx(*mx_ref.quantize_rows(y), z, d, f"act {act}")


def test_activation_references_and_the_polynomial_sensitivity():
    """act_ref64's tail-stable forms are clip_ref.act_fn's functions, and the figure act_delta's erf term
    rests on: |sum k a_k r^k| <= 3.5 on (0, 1] for the Abramowitz-Stegun coefficients."""
    t = np.linspace(-12, 12, 4801)
    for act in (1, 2, 3):
        assert np.all(np.abs(mc.act_ref64(act, t) - clip_ref.act_fn(mc.ACTS[act], t)) <= 4e-15)
    a = np.array([0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429])
    r = np.linspace(0, 1, 100001)[1:, None]
    k = np.arange(1, 6)
    assert np.abs((k * a * r ** k).sum(-1)).max() <= 3.5
    assert np.abs((a * r ** k).sum(-1)).max() <= 1 + 1e-6  # P <= 1: Q <= E


@EACH_SHAPE
def test_storeq_cases_reject_the_mutants(M, N, K):
    """Without an activation the comparison is ==: the neighbouring tile's bias slice, and the last row under
    another row's block amax, change bytes (and fail check_mx at delta 0 as well)."""
    c = mc.storeq_case(M, N, K)
    muts = [("partner amax", mc.mutant_partner_amax(c))]
    if N > 128:
        muts.append(("neighbour bias", mc.mutant_neighbour_bias(c)))
    for what, (q, s) in muts:
        assert not (np.array_equal(q, c.rq) and np.array_equal(s, c.rs)), what
        assert rejected(q, s, c.t, 0.0), what
    q, s = mc.mutant_partner_amax(c)
    assert np.array_equal(q[:-1], c.rq[:-1]) and not np.array_equal(s[-1], c.rs[-1])
    # with an activation, through the interval check
    for act in (1, 2, 3):
        y = mc.act_emulate_f32(act, c.t32)
        e_lo, e_hi = mc.scale_range(c.z(act), c.delta(act))
        one = np.argwhere((e_lo == e_hi) & (e_lo > -127))
        r, b = one[len(one) // 2]
        assert counts(rejected(*mc.mutant_scale_plus_one(y, r, b), c.z(act), c.delta(act)))[0] == 1
        assert rejected(*mc.mutant_amax_of_16(y), c.z(act), c.delta(act))
        assert rejected(*mc.mutant_truncate(y), c.z(act), c.delta(act))


# ---- the walk --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [MI355X_CUS, 304, 64])
def test_walk_shape(cus):
    """The walk shape gives some block three tiles on both MX tiles, and its sums are exact: no partial sum
    reaches 2^24 in units of the smallest term (integers: 16 K; storeq_case: exact_sum_bound)."""
    M, N, K = mc.walk_shape(cus)
    assert M % 128 == 104 and N % 128 == 32 and -(-N // 128) == 33
    for tile in (2, 3):
        per = mc.walk_tiles_per_block(M, N, tile, cus)
        assert max(per) >= 3 and min(per) >= 1, (tile, max(per), min(per))
    assert 16 * K + 64 < 2 ** 24 and mc.exact_sum_bound(K) < 2 ** 24
    if cus == MI355X_CUS:
        assert (M, N, K) == (4072, 4128, 256)


def test_walk_case_meets_the_caps():
    """The quantizing epilogue's case at the walk shape (256 CUs): the constructor's assertions hold, and
    QuickGELU, the activation the walk test runs, leaves the inputs under the caps."""
    c = mc.storeq_case(*mc.walk_shape(MI355X_CUS))
    blocks, elements = mc.ambiguity(c.z(1), c.delta(1))
    print(f"\n[mx] storeq walk {c.M}x{c.N}x{c.K} seed {c.seed}: {c.props}; act 1: ambiguous blocks {blocks:.4%} "
          f"elements {elements:.4%}")
    assert blocks <= mc.ACT_CAPS[0] and elements <= mc.ACT_CAPS[1]
