"""The embedding index's storage types without a GPU: the rounding rule of include/clipgpu.h as numpy
helpers (pinned against torch's casts on an input that holds every special class), the create-time
errors of clipgpu_index_create_ex, and the route hook's argument check.

tests/test_gpu_index_dtypes.py adds the rows built here to a 16-bit index and compares what the
device stored with these helpers, bit for bit."""
import ctypes

import numpy as np
import pytest

E_SPECIAL = 16


def round_f16(x):
    """f32 -> f16 -> f32, round to nearest even; subnormals kept, |x| >= 65520 -> inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def round_bf16(x):
    """f32 -> bf16 -> f32 by the usual bit formula: add 0x7fff + (bit 16), cut the low half; a NaN is
    kept (quiet bit set, so cutting cannot turn it into an infinity)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    r = np.where(np.isnan(x), (b & 0xFFFF0000) | 0x00400000, r)
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


ROUND = {"f16": round_f16, "bf16": round_bf16}


def nextafter32(x, to):
    return np.nextafter(np.float32(x), np.float32(to))


# name -> values; every class the header's rule speaks of
SPECIAL = {
    # exactly halfway between two neighbours of the 16-bit type; the even neighbour is below / above
    "f16_half_down": [1 + 2.0**-11, -(1 + 2.0**-11), 1024 + 0.5],
    "f16_half_up": [1 + 3 * 2.0**-11, -(1 + 3 * 2.0**-11), 1025 + 0.5],
    "bf16_half_down": [1 + 2.0**-8, -(1 + 2.0**-8), 256 + 1.0],
    "bf16_half_up": [1 + 3 * 2.0**-8, -(1 + 3 * 2.0**-8), 258 + 1.0],
    # the mantissa is all ones and rounds up: the carry goes into the exponent
    "f16_carry": [2 - 2.0**-12, -(4 - 2.0**-11), 2 - 2.0**-11],
    "bf16_carry": [2 - 2.0**-9, -(4 - 2.0**-8), 2 - 2.0**-8],
    # f16 subnormals: representable ones, one halfway (1.5 * 2^-24 -> 2 * 2^-24), and around 2^-25,
    # the largest value that still rounds to 0 (the tie goes to the even 0)
    "f16_subnormal": [2.0**-24, 3 * 2.0**-24, -(2.0**-15), 1023 * 2.0**-24, 1.5 * 2.0**-24, 2.0**-14 - 2.0**-24],
    "f16_to_zero": [2.0**-25, -(2.0**-25), 2.0**-30],
    "f16_just_above_zero": [float(nextafter32(2.0**-25, 1)), -float(nextafter32(2.0**-25, 1))],
    # the largest finite f16, the largest f32 that still rounds to it, the smallest that rounds to inf
    "f16_max": [65504.0, -65504.0, float(nextafter32(65520.0, 0))],
    "f16_to_inf": [65520.0, -65520.0, 1e6],
    "bf16_to_inf": [float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max)],
    "zeros": [0.0, -0.0],
    "infs": [np.inf, -np.inf],
    "nans": [np.nan, float(np.array([0xFFC00001], np.uint32).view(np.float32)[0]),
             float(np.array([0x7F800001], np.uint32).view(np.float32)[0])],
}


def special_values():
    return np.concatenate([np.asarray(v, np.float32) for v in SPECIAL.values()])


def special_rows():
    """[n][E_SPECIAL] f32: the special values, then ordinary ones to fill the rows."""
    v = special_values()
    rng = np.random.default_rng(42)
    n = -(-(len(v) + 150) // E_SPECIAL)  # a dozen rows
    fill = rng.standard_normal(n * E_SPECIAL - len(v)).astype(np.float32) * np.float32(3.0)
    return np.concatenate([v, fill]).reshape(n, E_SPECIAL)


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
