"""The embedding index's storage types without a GPU: the rounding rule of include/clipgpu.h as the numpy
helpers of tests/index_cases.py (pinned here against torch's casts on an input that holds every special
class), the create-time errors of clipgpu_index_create_ex, and the route hook's argument check.

tests/test_gpu_index_dtypes.py adds the same rows to a 16-bit index and compares what the device stored
with these helpers, bit for bit."""
import ctypes

import numpy as np
import pytest

from tests.index_cases import E_SPECIAL, ROUND, SPECIAL, nextafter32, round_bf16, round_f16, special_rows, \
    special_values


def neighbours(x, dt):
    """The two neighbours of the 16-bit type around a finite f32 x, in f64, and their low mantissa bits."""
    if dt == "f16":
        lo = np.float16(x) if np.float64(np.float16(x)) <= np.float64(x) else np.nextafter(np.float16(x), np.float16(-np.inf))
        hi = np.nextafter(lo, np.float16(np.inf))
        return np.float64(lo), np.float64(hi), int(lo.view(np.uint16)) & 1, int(hi.view(np.uint16)) & 1
    b = int(np.float32(x).view(np.uint32))
    lo_b, hi_b = b & 0xFFFF0000, (b & 0xFFFF0000) + 0x10000  # towards zero / away from zero
    lo = np.float64(np.array([lo_b], np.uint32).view(np.float32)[0])
    hi = np.float64(np.array([hi_b], np.uint32).view(np.float32)[0])
    return lo, hi, (lo_b >> 16) & 1, (hi_b >> 16) & 1


def test_the_input_holds_every_class():
    """The special values are what their names say (exact f64 arithmetic on the CPU), so the
    comparisons below and on the GPU do test the rule's corners."""
    for dt in ("f16", "bf16"):
        rnd = ROUND[dt]
        for name, even_is in ((dt + "_half_down", "lo"), (dt + "_half_up", "hi")):
            for x in SPECIAL[name]:
                x = np.float32(x)
                assert np.float64(x) == float(x)
                lo, hi, lo_odd, hi_odd = neighbours(abs(x), dt)
                assert (lo + hi) / 2 == np.float64(abs(x)), (name, x)  # exactly halfway
                assert (lo_odd, hi_odd) == ((0, 1) if even_is == "lo" else (1, 0)), (name, x)
                assert np.float64(abs(rnd(np.array([x]))[0])) == (lo if even_is == "lo" else hi), (name, x)
        for x in SPECIAL[dt + "_carry"]:
            x = np.float32(x)
            r = rnd(np.array([x]))[0]
            # the result is a power of two above |x|: another exponent than x's
            assert abs(r) > abs(x) and np.frexp(abs(r))[0] == 0.5 and np.frexp(abs(r))[1] == np.frexp(abs(x))[1] + 1
    sub = round_f16(np.asarray(SPECIAL["f16_subnormal"], np.float32))
    assert (np.abs(sub) < 2.0**-14).all() and (sub != 0).all()  # f16 subnormals, kept
    assert sub[4] == np.float32(2 * 2.0**-24)
    assert (round_f16(np.asarray(SPECIAL["f16_to_zero"], np.float32)) == 0).all()
    assert np.signbit(round_f16(np.asarray(SPECIAL["f16_to_zero"], np.float32)))[1]  # -2^-25 -> -0.0
    assert (np.abs(round_f16(np.asarray(SPECIAL["f16_just_above_zero"], np.float32))) == np.float32(2.0**-24)).all()
    assert (np.abs(round_f16(np.asarray(SPECIAL["f16_max"], np.float32))) == 65504).all()
    assert np.isinf(round_f16(np.asarray(SPECIAL["f16_to_inf"], np.float32))).all()
    assert nextafter32(65520.0, 0) < 65520 and SPECIAL["f16_to_inf"][0] == 65520.0  # the smallest that rounds to inf
    assert np.isinf(round_bf16(np.asarray(SPECIAL["bf16_to_inf"], np.float32))).all()
    z = np.asarray(SPECIAL["zeros"], np.float32)
    assert (z == 0).all() and list(np.signbit(z)) == [False, True]
    assert np.isinf(np.asarray(SPECIAL["infs"], np.float32)).all()
    assert np.isnan(np.asarray(SPECIAL["nans"], np.float32)).all()
    rows = special_rows()
    assert rows.shape[1] == E_SPECIAL and rows.dtype == np.float32
    flat = rows.ravel()
    n = len(special_values())
    assert np.array_equal(flat[:n].view(np.uint32), special_values().view(np.uint32))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_numpy_rounding_is_torchs(dt):
    import torch
    x = special_rows()
    got = ROUND[dt](x)
    want = torch.tensor(x).to(torch.float16 if dt == "f16" else torch.bfloat16).float().numpy()
    nan = np.isnan(x)
    assert nan.sum() == len(SPECIAL["nans"])
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)  # NaN stays NaN, nothing else is
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])  # signs of zeros and infs included
    assert np.signbit(got.ravel()[list(special_values().view(np.uint32)).index(0x80000000)])  # -0.0 stays -0.0


@pytest.mark.parametrize("dtype", [3, -1])
def test_unknown_dtype_is_refused(dtype):
    from open_clip_inference import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.clipgpu_index_create_ex(0, 64, 8, dtype, ctypes.byref(h)) == 1  # CLIPGPU_ERR_INVALID
    assert "unknown index dtype" in L.clipgpu_last_error().decode()
    assert not h.value


def test_python_refuses_an_unknown_dtype():
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    with pytest.raises((ValueError, ClipError)):
        EmbeddingIndex(64, 8, dtype="f64")


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("E,capacity,null_out,msg", [(0, 8, False, "embedding dim must be a multiple of 16"),
                                                     (24, 8, False, "embedding dim must be a multiple of 16"),
                                                     (64, 0, False, "capacity must be positive"),
                                                     (64, 8, True, "NULL out")])
def test_create_ex_keeps_the_create_time_errors(E, capacity, null_out, msg, dtype):
    from open_clip_inference import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.clipgpu_index_create_ex(0, E, capacity, dtype, None if null_out else ctypes.byref(h))
    assert rc == 1
    assert msg in L.clipgpu_last_error().decode()
    assert not h.value
    assert L.clipgpu_index_dtype(None) == -1


def test_route_hook_takes_0_1_2():
    from open_clip_inference import _lib
    L = _lib.lib()
    try:
        for bad in (3, -1):
            assert L.clipgpu_test_topk_route(bad) == 1 and b"route must be" in L.clipgpu_last_error()
        for ok in (1, 2, 0):
            assert L.clipgpu_test_topk_route(ok) == 0
    finally:
        L.clipgpu_test_topk_route(0)
