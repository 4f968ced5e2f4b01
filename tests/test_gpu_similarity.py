"""The similarity kernels (csrc/kernels/similarity.hip) on the GPU, through clipgpu_similarity (the
`similarity` wrapper) and clipgpu_similarity_device.  The embedding index's tests take these kernels'
logits and sigmoids as their expected result bit for bit, so this file holds the kernels themselves, to
tests/similarity_cases.py (checked on the CPU by tests/test_cpu_similarity_cases.py):

  exact    logits on integer operands (one fmaf of an exact dot), the coordinate stamp, the K census, the
           independence of out[i][j] from everything but img[i] and txt[j], softmaxes whose exponentials
           are exactly 0 or 1, saturated sigmoids, the device form against the host form: uint32 views;
  bounded  logits of unit rows against float64 (similarity_cases.logit_bound), softmax and sigmoid against
           float64 on the kernels' own f32 logits (index_probs_cases.bound_matrix, SIGMOID_BOUND).
There is no other tolerance."""
import numpy as np
import pytest

from tests import similarity_cases as cases

pytestmark = pytest.mark.gpu

F = np.float32
ACT = {"softmax": 0, "sigmoid": 1, "logits": 2}


def sim(a, b, scale=1.0, bias=0.0, act="logits", axis=1):
    from open_clip_inference.engine import similarity
    out = similarity(a, b, scale, bias, act, axis)
    assert out.dtype == F and out.shape == (len(a), len(b))
    return out


def same_bits(got, want, what=""):
    assert got.dtype == F and want.dtype == F and got.shape == want.shape, what
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (what, f"{len(bad)} of {got.size} differ", [
        (tuple(int(x) for x in ij), float(got[tuple(ij)]), float(want[tuple(ij)])) for ij in bad[:5]])


# ---- 1. exact logits on integer operands ---------------------------------------------------------------------
@pytest.mark.parametrize("ni,nt,E", cases.INT_SHAPES)
def test_integer_logits_are_the_exact_dot_through_one_fmaf(ni, nt, E):
    a, b = cases.int_case(ni, nt, E)
    for scale, bias in cases.PAIRS:
        same_bits(sim(a, b, scale, bias), cases.logits_oracle(a, b, scale, bias), (scale, bias))


@pytest.mark.parametrize("scale,bias", cases.FUSED_PAIRS)
def test_the_logit_is_rounded_once_not_twice(scale, bias):
    """round_f32(d * scale + bias), not f32(f32(d) * scale) + bias: the two differ on about 30 % of this
    case's elements, and the kernel gives the first on all of them."""
    a, b = cases.int_case(129, 130, 80)
    d = cases.int_dot(a, b)
    once, twice = cases.fused(d, scale, bias), cases.two_roundings(d, scale, bias)
    tell = once.view(np.uint32) != twice.view(np.uint32)
    assert tell.mean() >= 0.10
    got = sim(a, b, scale, bias)
    as_twice = int((got.view(np.uint32)[tell] == twice.view(np.uint32)[tell]).sum())
    assert as_twice == 0, f"{as_twice} of {int(tell.sum())} telling elements carry the two-rounding value"
    same_bits(got, once)


@pytest.mark.parametrize("ni,nt", cases.STAMP_SHAPES)
def test_every_element_carries_its_own_coordinates(ni, nt):
    a, b = cases.stamp_case(ni, nt)
    wrong = cases.stamp_diff(sim(a, b), ni, nt)
    assert wrong is None, wrong


@pytest.mark.parametrize("E", cases.CENSUS_E)
def test_every_k_position_counts_once(E):
    a, b = cases.census_case(E)
    same_bits(sim(a, b), cases.census_expected(E))


# ---- 2. position independence on ordinary data ---------------------------------------------------------------
@pytest.mark.parametrize("E", cases.UNIT_E)
def test_an_element_depends_on_its_row_and_column_alone(E):
    """Logits of row and column subsets, and the softmax of one row / one column alone, are bit for bit
    those of the full call."""
    a, b = cases.unit_case(E)
    ni, nt = len(a), len(b)
    L = sim(a, b, 100.0, 0.0)
    for i in (0, 64, ni - 1):
        same_bits(sim(a[i:i + 1], b, 100.0, 0.0), L[i:i + 1], f"row {i}")
    for j in (0, 63, nt - 1):
        same_bits(sim(a, b[j:j + 1], 100.0, 0.0), L[:, j:j + 1], f"column {j}")
    same_bits(sim(a[63:66], b, 100.0, 0.0), L[63:66], "rows 63:66")
    same_bits(sim(a, b[60:70], 100.0, 0.0), L[:, 60:70], "columns 60:70")
    same_bits(sim(a[63:66], b[60:70], 100.0, 0.0), L[63:66, 60:70], "rows 63:66 x columns 60:70")
    P1, P0 = sim(a, b, 100.0, 0.0, "softmax", 1), sim(a, b, 100.0, 0.0, "softmax", 0)
    for i in (0, 3, 4, ni - 1):
        same_bits(sim(a[i:i + 1], b, 100.0, 0.0, "softmax", 1), P1[i:i + 1], f"softmax of row {i}")
    for j in (0, 63, 64, nt - 1):
        same_bits(sim(a, b[j:j + 1], 100.0, 0.0, "softmax", 0), P0[:, j:j + 1], f"softmax of column {j}")


@pytest.mark.parametrize("E", cases.UNIT_E)
def test_swapping_the_operands_transposes_the_bits(E):
    """Guaranteed by the kernel: img and txt are staged by the same code into sA / sB ([row][k], k slabs of
    16), lane (r, q) hands the MFMA sA[row][kk + q] and sB[col][kk + q], and out[i][j] accumulates the
    products a[i][k] * b[j][k] for k ascending in both calls; a product does not depend on which operand
    is which.  (The index's self-join relies on the same fact.)"""
    a, b = cases.unit_case(E)
    for scale, bias in cases.BOUND_PAIRS:
        same_bits(sim(b, a, scale, bias), np.ascontiguousarray(sim(a, b, scale, bias).T), (scale, bias))


# ---- 3. the derived bound for real-valued logits -------------------------------------------------------------
@pytest.mark.parametrize("E", cases.UNIT_E)
@pytest.mark.parametrize("scale,bias", cases.BOUND_PAIRS)
def test_unit_row_logits_are_within_the_derived_bound_of_float64(E, scale, bias):
    a, b = cases.unit_case(E)
    ref, mags = cases.logits64(a, b, scale, bias)
    bound = cases.logit_bound(E, scale, mags, ref)
    err = np.abs(sim(a, b, scale, bias).astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / bound).max())


# ---- 4. softmax and sigmoid on the kernels' own logits -------------------------------------------------------
@pytest.mark.parametrize("scale", cases.SOFTMAX_SCALES)
@pytest.mark.parametrize("ni,nt", cases.ROWS_KERNEL_SHAPES)
def test_softmax_over_the_labels_is_within_the_matrix_bound(ni, nt, scale):
    a, b = cases.unit_case(64, ni, nt)
    cases.check_softmax(sim(a, b, scale, 0.0, "softmax", 1), sim(a, b, scale, 0.0), 1)


@pytest.mark.parametrize("scale", cases.SOFTMAX_SCALES)
@pytest.mark.parametrize("ni,nt", cases.COLS_KERNEL_SHAPES)
def test_softmax_over_the_images_is_within_the_matrix_bound(ni, nt, scale):
    a, b = cases.unit_case(64, ni, nt)
    cases.check_softmax(sim(a, b, scale, 0.0, "softmax", 0), sim(a, b, scale, 0.0), 0)


@pytest.mark.parametrize("ni,nt,axis", cases.PATTERN_SHAPES)
def test_softmax_of_zeros_and_minus_128_is_exact(ni, nt, axis):
    """expf is exactly 1 and 0, the sum an exact count c: f32(1) / f32(c) or 0, with a line that holds a
    single zero (probability 1.0) and an all-equal line (1 / n)."""
    a, b, L = cases.pattern_case(ni, nt, axis)
    same_bits(sim(a, b, cases.PATTERN_SCALE, 0.0), L, "logits")
    same_bits(sim(a, b, cases.PATTERN_SCALE, 0.0, "softmax", axis), cases.exact_softmax(L, axis))


@pytest.mark.parametrize("scale,bias", cases.BOUND_PAIRS)
def test_sigmoid_is_within_one_expf_one_add_and_one_division(scale, bias):
    a, b = cases.unit_case(64)
    cases.check_sigmoid(sim(a, b, scale, bias, "sigmoid"), sim(a, b, scale, bias))


def test_sigmoid_saturates_exactly():
    a, b, want = cases.saturation_case()
    same_bits(sim(a, b, 128.0, 0.0), cases.logits_oracle(a, b, 128.0, 0.0), "logits")
    same_bits(sim(a, b, 128.0, 0.0, "sigmoid"), want)


def all_nan_except(got, base, rows=None, cols=None):
    """Row(s) / column(s) NaN throughout, everything else bit for bit as in `base`."""
    nan = np.zeros(got.shape, bool)
    if rows is not None:
        nan[rows] = True
    if cols is not None:
        nan[:, cols] = True
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], base.view(np.uint32)[~nan])


@pytest.mark.parametrize("i", [3, cases.UNIT_NI - 1])
def test_a_nan_in_an_image_row_stays_in_its_row(i):
    """Row ni - 1 is also the row the kernel stages in place of the rows past the end."""
    a, b = cases.unit_case(64)
    bad = a.copy()
    bad[i, 5] = np.nan
    for act, axis in (("logits", 1), ("sigmoid", 1), ("softmax", 1)):
        all_nan_except(sim(bad, b, 100.0, 0.0, act, axis), sim(a, b, 100.0, 0.0, act, axis), rows=i)
    assert np.isnan(sim(bad, b, 100.0, 0.0, "softmax", 0)).all()


@pytest.mark.parametrize("j", [64, cases.UNIT_NT - 1])
def test_a_nan_in_a_label_row_stays_in_its_column(j):
    a, b = cases.unit_case(64)
    bad = b.copy()
    bad[j, 7] = np.nan
    for act, axis in (("logits", 1), ("sigmoid", 1), ("softmax", 0)):
        all_nan_except(sim(a, bad, 100.0, 0.0, act, axis), sim(a, b, 100.0, 0.0, act, axis), cols=j)
    assert np.isnan(sim(a, bad, 100.0, 0.0, "softmax", 1)).all()


def test_an_infinite_logit_makes_its_softmax_line_nan():
    """One element whose dot is finite (3e38) and whose logit at scale 100 is +inf: exp(inf - inf) is NaN,
    as index_probs_cases.oracle states for the fused path; every other line is held to the bound."""
    a, b = (x.copy() for x in cases.unit_case(64))
    i, j = 66, 101
    b[:, 0] = 0
    b[j, 0] = 1
    a[i, 0] = 3e38
    L = sim(a, b, 100.0, 0.0)
    inf = np.zeros(L.shape, bool)
    inf[i, j] = True
    assert np.array_equal(np.isposinf(L), inf) and np.isfinite(L[~inf]).all()
    P1, P0 = sim(a, b, 100.0, 0.0, "softmax", 1), sim(a, b, 100.0, 0.0, "softmax", 0)
    assert np.isnan(P1[i]).all() and np.isnan(P0[:, j]).all()
    assert np.isnan(P1).sum() == L.shape[1] and np.isnan(P0).sum() == L.shape[0]
    cases.check_softmax(P1, L, 1)
    cases.check_softmax(P0, L, 0)


# ---- 5. clipgpu_similarity_device ----------------------------------------------------------------------------
def sim_device(d_img, ni, d_txt, nt, E, scale, bias, act, axis, d_out, stream=None):
    from open_clip_inference import _lib
    _lib.check(_lib.lib().clipgpu_similarity_device(d_img, ni, d_txt, nt, E, scale, bias, act, axis, d_out, stream))


MODES = [("logits", 1), ("sigmoid", 1), ("softmax", 1), ("softmax", 0)]


def test_the_device_form_gives_the_bits_of_the_host_form():
    import torch
    a, b = cases.unit_case(80)
    ni, nt = len(a), len(b)
    da, db = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    out = torch.empty((ni, nt), dtype=torch.float32, device="cuda")
    for act, axis in MODES:
        out.fill_(float("nan"))
        sim_device(da.data_ptr(), ni, db.data_ptr(), nt, 80, 117.33, -12.9, ACT[act], axis, out.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same_bits(out.cpu().numpy(), sim(a, b, 117.33, -12.9, act, axis), (act, axis))


@pytest.mark.parametrize("ni,nt", [(65, 130), (5, 63)])
def test_the_device_form_writes_nothing_outside_out(ni, nt):
    """out lies between two sentinel rows of one allocation; every activation leaves both intact."""
    import torch
    a, b = cases.unit_case(64, ni, nt)
    da, db = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    sentinel = 24576.0
    for act, axis in MODES:
        buf = torch.full((ni + 2, nt), sentinel, dtype=torch.float32, device="cuda")
        sim_device(da.data_ptr(), ni, db.data_ptr(), nt, 64, 100.0, 0.0, ACT[act], axis, buf[1].data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[0] == sentinel).all() and (got[-1] == sentinel).all(), (act, axis)
        same_bits(np.ascontiguousarray(got[1:-1]), sim(a, b, 100.0, 0.0, act, axis), (act, axis))


@pytest.mark.parametrize("which", ["current", "side"])
def test_the_device_form_runs_in_stream_order(which):
    """On the stream, with no synchronisation in between: a 3 ms delay, the copy that replaces NaN-filled
    inputs by the real ones, the call, a clone of out.  A launch on another stream reads the NaNs."""
    import torch
    from open_clip_inference import _lib
    a, b = cases.unit_case(80)
    ni, nt = len(a), len(b)
    real_a, real_b = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    da, db = torch.full_like(real_a, float("nan")), torch.full_like(real_b, float("nan"))
    out = torch.full((ni, nt), float("nan"), dtype=torch.float32, device="cuda")
    probe = torch.zeros(2, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream() if which == "current" else torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _lib.check(_lib.lib().clipgpu_test_clock_probe(s.cuda_stream, 3000, probe.data_ptr()))
        da.copy_(real_a, non_blocking=True)
        db.copy_(real_b, non_blocking=True)
        sim_device(da.data_ptr(), ni, db.data_ptr(), nt, 80, 100.0, 0.0, ACT["softmax"], 1, out.data_ptr(),
                   s.cuda_stream)
        got = out.clone()
    s.synchronize()
    assert int(probe[1]) >= 3000 * 100  # the delay ran (100 MHz ticks)
    same_bits(got.cpu().numpy(), sim(a, b, 100.0, 0.0, "softmax", 1))


def test_the_device_form_refuses_bad_arguments():
    import torch
    from open_clip_inference.error import InferenceError, ShapeError
    d = torch.zeros((4, 32), dtype=torch.float32, device="cuda")
    out = torch.full((4, 4), 7.0, dtype=torch.float32, device="cuda")
    p, o = d.data_ptr(), out.data_ptr()
    for ni, nt in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(InferenceError, match="Empty batch"):
            sim_device(p, ni, p, nt, 32, 1.0, 0.0, 2, 1, o)
    for E in (0, 8, 24):
        with pytest.raises(ShapeError, match="Shape error: embedding dim must be a multiple of 16"):
            sim_device(p, 4, p, 4, E, 1.0, 0.0, 2, 1, o)
    for act, axis in ((-1, 1), (3, 1), (2, 2), (0, 2), (0, -1)):
        with pytest.raises(InferenceError, match="bad activation / axis"):
            sim_device(p, 4, p, 4, 32, 1.0, 0.0, act, axis, o)
    for args in ((None, p, o), (p, None, o), (p, p, None)):
        with pytest.raises(InferenceError, match="NULL buffer"):
            sim_device(args[0], 4, args[1], 4, 32, 1.0, 0.0, 2, 1, args[2])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()  # nothing was launched


def test_more_image_rows_than_the_grid_holds_is_a_shape_error():
    """launch_similarity takes at most 65535 * 64 image rows (one grid row per 64); clipgpu.h states the
    limit, and beyond it the caller gets the Shape error of the other size checks, not a HIP error.  The
    buffers are real (256 MiB of zeros) but nothing is launched."""
    import torch
    from open_clip_inference.error import ShapeError
    n = 1 << 22
    d = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
    one = torch.zeros((1, 16), dtype=torch.float32, device="cuda")
    out = torch.full((n, 1), 7.0, dtype=torch.float32, device="cuda")
    for rows in (n, 65535 * 64 + 1):
        with pytest.raises(ShapeError, match="Shape error: similarity matrix too large"):
            sim_device(d.data_ptr(), rows, one.data_ptr(), 1, 16, 1.0, 0.0, 2, 1, out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
