"""The derived bounds of tests/test_gpu_rowwise.py, checked without a GPU: a numpy-f32 emulation of each
kernel's arithmetic, on the very inputs the GPU tests use, must stay inside the bound against the fp64
reference.  If it does not, the bound's derivation is wrong -- not the kernel."""
import numpy as np
import pytest

from tests import rowwise_cases as rc
from tests.rowwise_cases import BF16, F16

LN_DIMS = [4, 128, 260, 1024, 1028, 1152, 1280]


@pytest.mark.parametrize("x16", [0, 1])
@pytest.mark.parametrize("D", LN_DIMS)
def test_f32_two_pass_layernorm_is_inside_the_bounds(D, x16):
    w, b = rc.ln_params(D, D)
    x = rc.ln_rows_input(37, D, D + x16, x16)
    out, stats = rc.ln_emulate_f32(x, w, b)
    rc.check_ln32(out, x, w, b)
    rc.check_stats(stats, x)
    for dtype in (BF16, F16):
        rc.check_ln16(dtype, rc.round16(out, dtype), x, w, b)
        # ln_1 of an f16-stored ln_pre output (the stems): the stored row is the second LN's input
        y = rc.stream(out, x16)
        h, hstats = rc.ln_emulate_f32(y, b + 1, w - 1)
        rc.check_ln16(dtype, rc.round16(h, dtype), y, b + 1, w - 1)
        rc.check_stats(hstats, y)


def test_bounds_reject_an_unbiased_variance_and_a_one_pass_variance():
    """The errors the 16-bit bars forgave: at D = 1280 a variance over D - 1 moves rstd by 4e-4 relative
    (the statistics bound is 3.8e-6), and a one-pass E[x^2] - mean^2 in f32 loses a row of |mean| = 100 std."""
    D = 1280
    x = rc.ln_rows_input(37, D, D, 0)
    _, stats = rc.ln_emulate_f32(x, np.ones(D), np.zeros(D))
    x64 = x.astype(np.float64)
    unbiased = stats.copy()
    unbiased[:, 1] = 1.0 / np.sqrt(x64.var(-1, ddof=1) + rc.EPS)
    with pytest.raises(AssertionError):
        rc.check_stats(unbiased, x)
    one_pass = stats.copy()
    m = x.mean(-1, dtype=np.float32)
    one_pass[:, 1] = 1.0 / np.sqrt(np.maximum((x * x).mean(-1, dtype=np.float32) - m * m, 0) + np.float32(rc.EPS))
    with pytest.raises(AssertionError):
        rc.check_stats(one_pass, x)


@pytest.mark.parametrize("span", [60, 100, 3])
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B,N,H,hd", [(2, 1, 2, 64), (3, 17, 2, 8), (2, 257, 3, 72), (1, 1024, 2, 128)])
def test_f32_map_attention_is_inside_the_bound(B, N, H, hd, dtype, span):
    q, kv = rc.map_case(B, N, H, hd, dtype, span, N + hd)
    ref = rc.map_ref(q, kv, B, N, H, hd)
    got = rc.round16(rc.map_emulate_f32(q, kv, B, N, H, hd), dtype)
    assert np.all(np.abs(got - ref) <= rc.map_bound(dtype, ref, kv, H * hd))


@pytest.mark.parametrize("B,E", [(1, 1), (5, 63), (7, 65), (9, 512), (3, 1152)])
def test_f32_l2norm_is_inside_the_bound(B, E):
    for shift in range(3):
        x = rc.l2_rows(B, E, E, shift)
        ref = rc.l2_ref(x)
        assert np.all(np.abs(rc.l2_emulate_f32(x) - ref) <= 32 * rc.U * np.abs(ref))
