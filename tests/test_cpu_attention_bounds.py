"""The derived bound of tests/test_gpu_attention.py, checked without a GPU (tests/attention_cases.py).
On every (shape, type, mask, kind) the GPU file runs, a numpy-f32 emulation of the kernel that
launch_attention picks for the shape must stay inside the bound against the fp64 reference: if it does
not, the derivation is wrong, not the kernel.  And the bound must reject each mutant of the emulation on
cases of the same sweep: if one slips through, the inputs change, never the bound."""
import numpy as np
import pytest

from tests import attention_cases as ac
from tests.attention_cases import BF16, F16


def emulations_inside(N, HD, causal, dtype, kinds):
    for kind, span in kinds:
        case = ac.make_case(kind, span, N, HD, causal, dtype)
        case.check(ac.emulate_case(case))


@pytest.mark.parametrize("N,HD,causal,dtype", ac.WHOLE_PARAMS, ids=[ac.param_id(p) for p in ac.WHOLE_PARAMS])
def test_whole_row_emulation_is_inside_the_bound(N, HD, causal, dtype):
    assert not ac.is_tiled(N, HD)
    emulations_inside(N, HD, causal, dtype, ac.KINDS)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_whole_row_emulation_is_inside_the_bound_at_every_text_length(dtype):
    for N in ac.SWEEP_N:
        emulations_inside(N, 64, 1, dtype, ac.SWEEP_KINDS)


@pytest.mark.parametrize("N,HD,causal,dtype", ac.TILED_PARAMS, ids=[ac.param_id(p) for p in ac.TILED_PARAMS])
def test_online_emulation_is_inside_the_bound(N, HD, causal, dtype):
    assert ac.is_tiled(N, HD)
    emulations_inside(N, HD, causal, dtype, ac.KINDS)


def _marked(fn):
    """[(parameters as a dict)] of a test function with stacked parametrize marks."""
    sets = [{}]
    for mark in fn.pytestmark:
        names = [n.strip() for n in mark.args[0].split(",")]
        sets = [dict(s, **dict(zip(names, v if len(names) > 1 else (v,)))) for s in sets for v in mark.args[1]]
    return sets


def _random_input_cases():
    """The random inputs of tests/test_gpu_kernels.py's three attention tests, which hold the kernels to
    the same bound: every parameter set of each, with the test's own input function."""
    from tests import test_gpu_kernels as tk
    cases = []
    for fn, inputs in [(tk.test_attention, tk.attention_inputs), (tk.test_attention_large_batch, tk.attention_large_batch_inputs),
                       (tk.test_attention_tiled, tk.attention_tiled_inputs)]:
        for p in _marked(fn):
            cases.append(pytest.param(inputs, p, id=fn.__name__ + "-" + "-".join(f"{k}{v}" for k, v in p.items())))
    return cases


@pytest.mark.parametrize("inputs,p", _random_input_cases())
def test_emulation_is_inside_the_bound_on_the_random_inputs(inputs, p):
    """(Of a bench-sized batch the first, middle and last 8 sequences: its sequences are independent and
    drawn alike, and numpy takes ten seconds over 5600 heads.)"""
    HD, B, N = p.get("HD", 64), p["B"], p["N"]
    qkv = inputs(**p)
    if B > 24:
        qkv = np.concatenate([qkv[s * N:(s + 8) * N] for s in (0, B // 2, B - 8)])
        B = 24
    case = ac.packed_case("randn", qkv, B, N, p["H"], HD, p["causal"], p["dtype"])
    case.check(ac.emulate_case(case))


def test_both_schedules_agree_where_either_could_run():
    """The two emulations differ in schedule only: each is inside the bound on the other's shapes too."""
    for N, HD, causal, dtype in [(77, 64, 1, BF16), (256, 64, 0, F16), (257, 64, 1, F16), (65, 80, 0, BF16)]:
        for kind, span in ac.KINDS:
            case = ac.make_case(kind, span, N, HD, causal, dtype)
            for tiled in (False, True):
                case.check(ac.emulate(case.q, case.k, case.v, causal, dtype, tiled))


def in_the_sweep(kind, span, N, HD, causal, dtype):
    """Does tests/test_gpu_attention.py run this case?"""
    params = ac.TILED_PARAMS if ac.is_tiled(N, HD) else ac.WHOLE_PARAMS
    return (N, HD, causal, dtype) in params and (kind, span) in ac.KINDS


@pytest.mark.parametrize("mutant", ac.MUTANTS)
def test_the_bound_rejects(mutant):
    """Each mistake leaves the bound on named cases of the GPU sweep, on which the unmutated emulation is
    inside it."""
    assert ac.MUTANT_CASES[mutant]
    for args in ac.MUTANT_CASES[mutant]:
        assert in_the_sweep(*args), args
        case = ac.make_case(*args)
        case.check(ac.emulate_case(case))
        r, idx = case.worst(ac.emulate_case(case, mutant))
        assert r > 1.5, (mutant, case.name, r, idx)


def test_reference_against_a_direct_loop():
    """attn_ref and its A, S, V against per-query loops in fp64, causal and not."""
    rng = np.random.default_rng(5)
    B, N, H, HD = 2, 7, 2, 8
    q, k, v = (rng.standard_normal((B, N, H, HD)) for _ in range(3))
    for causal in (0, 1):
        ref, A, S, V = ac.attn_ref(q, k, v, causal)
        for b in range(B):
            for h in range(H):
                for i in range(N):
                    n = i + 1 if causal else N
                    s = k[b, :n, h] @ q[b, i, h] / np.sqrt(HD)
                    p = np.exp(s - s.max())
                    p /= p.sum()
                    assert np.allclose(ref[b, i, h], p @ v[b, :n, h], rtol=1e-12, atol=1e-14)
                    assert np.allclose(A[b, i, h], p @ np.abs(v[b, :n, h]), rtol=1e-12)
                    assert np.allclose(S[b, i, h, 0], (np.abs(k[b, :n, h]) @ np.abs(q[b, i, h])).max() / np.sqrt(HD))
                    assert np.allclose(V[b, i, h], np.abs(v[b, :n, h]).sum(0), rtol=1e-12)
    qkv = ac.pack(q, k, v)
    assert qkv.shape == (B * N, 3 * H * HD)
    for a, b_ in zip(ac.unpack(qkv, B, N, H, HD), (q, k, v)):
        assert np.array_equal(a, b_.astype(np.float32))
    assert np.array_equal(qkv[N + 2, H * HD + HD:H * HD + 2 * HD], k[1, 2, 1].astype(np.float32))


def test_inputs_reach_their_span():
    """The largest allowed |score| of every (sequence, head) is the kind's span (up to the 16-bit rounding
    of q and k).  Every score of `negative` is well below 0: -40 (0.5 * 4) / (1.5 * 8) = -6.7 from the
    ranges of the coefficients, less three deviations (15 % each) of q's noise against k."""
    for kind, span in ac.KINDS:
        for causal in (0, 1):
            q, k, _ = ac.make_inputs(kind, span, 2, 77, 3, 64, causal, F16)
            s = np.einsum("bihd,bjhd->bhij", q.astype(np.float64), k.astype(np.float64)) / 8
            s = np.where(ac.allowed_keys(77, causal), s, 0.0)
            assert np.allclose(np.abs(s).max((2, 3)), span, rtol=0.01), (kind, span, causal)
            if kind == "negative":
                assert np.where(ac.allowed_keys(77, causal), s, -np.inf).max() < -6.7 * (1 - 3 * 0.15)
