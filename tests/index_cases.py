"""Helpers shared by the embedding index's tests (tests/test_cpu_index_*.py, tests/test_gpu_index_*.py,
tests/test_gpu_topk*.py): inputs, the sorted-logits oracle, exact comparisons, the library's test hooks and
the numpy model of the 16-bit rounding rule of include/clipgpu.h.  The probability search's oracle and error
bound are tests/index_probs_cases.py.

The library is imported inside the functions that need it, so this module imports without a GPU."""
from contextlib import contextmanager

import numpy as np


# ---- inputs ---------------------------------------------------------------------------------------------
def unit_rows(rng, n, E):
    x = rng.standard_normal((n, E)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def tied_gallery(rng, N, E=64):
    base = unit_rows(rng, 8, E)
    d = base.astype(np.float64) @ base.astype(np.float64).T
    return base, base[rng.integers(0, 8, N)], d


def pattern(n):
    """Rows 0, 3, 6, 9, 10, 12, ...: T F F T F F T F in the first byte, no palindrome at any length >= 2."""
    i = np.arange(n)
    return (i % 3 == 0) | (i % 7 == 3)


# ---- the expected result, from the full logits matrix ---------------------------------------------------
def expected(q, g, k, scale, bias):
    from open_clip_inference.engine import similarity
    L = similarity(q, g, scale, bias, "logits", 1)
    idx = np.argsort(-L, axis=1, kind="stable")[:, :k]
    score = np.take_along_axis(L, idx, 1)
    if idx.shape[1] < k:  # fewer rows than k: (-1, -inf) padding
        pad = k - idx.shape[1]
        idx = np.concatenate([idx, np.full((len(q), pad), -1, np.int64)], 1)
        score = np.concatenate([score, np.full((len(q), pad), -np.inf, np.float32)], 1)
    return idx.astype(np.int64), score


def padding(Q, k):
    return np.full((Q, k), -1, np.int64), np.full((Q, k), -np.inf, np.float32)


def logits_oracle(L, allow, k):
    """From the full logits matrix: a stable descending sort over the allowed columns."""
    A = np.flatnonzero(allow)
    order = np.argsort(-L[:, A], axis=1, kind="stable")[:, :k]
    idx, score = A[order].astype(np.int64), np.take_along_axis(L[:, A], order, 1)
    pad = k - idx.shape[1]
    if pad > 0:
        pi, ps = padding(len(L), pad)
        idx, score = np.concatenate([idx, pi], 1), np.concatenate([score, ps], 1)
    return idx, np.ascontiguousarray(score, dtype=np.float32)


# ---- exact comparisons ----------------------------------------------------------------------------------
def assert_same(got, want, what=""):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


def bits_equal_with_nans(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- searches and the library's test hooks --------------------------------------------------------------
def search_once(q, g, k, scale=100.0, bias=0.0):
    from open_clip_inference import EmbeddingIndex
    with EmbeddingIndex(g.shape[1], len(g)) as ix:
        ix.add(g)
        assert len(ix) == len(g)
        return ix.search(q, k, scale, bias)


def search16(q, g, k, dt, scale=100.0, bias=0.0):
    from open_clip_inference import EmbeddingIndex
    with EmbeddingIndex(g.shape[1], len(g), dtype=dt) as ix:
        ix.add(g)
        return ix.search(q, k, scale, bias)


def span_cols(cols):
    from open_clip_inference import _lib
    _lib.check(_lib.lib().clipgpu_test_topk_span_cols(cols))


@contextmanager
def route(r):
    from open_clip_inference import _lib
    _lib.check(_lib.lib().clipgpu_test_topk_route(r))
    try:
        yield
    finally:
        _lib.check(_lib.lib().clipgpu_test_topk_route(0))


def routes_for(Q):
    """Both phase-1 kernels where the few-query one can run, else the default dispatch."""
    return (1, 2) if Q <= 16 else (0,)


# ---- the rounding rule of a 16-bit index, and an input that holds every special class -------------------
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
