"""The host side of the embedding index's range search and self-join (no GPU): the three new symbols of
libclipgpu.so with their declared argument types, the refusals that are made before any device call, the
argument checks that EmbeddingIndex makes before it reaches the library, and the oracle of
tests/index_range_cases.py itself on a hand-written matrix."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import index_range_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P = ctypes.c_void_p
C = {"clipgpu_index*": P, "const int64_t*": P, "int64_t*": P, "int32_t*": P, "uint64_t*": P, "const float*": P,
     "float*": P, "const uint32_t*": P, "void*": P, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
     "int": ctypes.c_int}
NEW = {"clipgpu_index_range_search_device": 13, "clipgpu_index_range_search": 12, "clipgpu_index_self_join": 10}
INVALID = 1  # CLIPGPU_ERR_INVALID
NAN, INF = float("nan"), float("inf")


def declared(name):
    """(return type, argument types) of `name` as include/clipgpu.h declares it, as ctypes types."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipgpu.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    args = [C[" ".join(a.split()[:-1])] for a in m.group(2).split(",")]  # drop the parameters' names
    return C[m.group(1)], args


@pytest.mark.parametrize("name", sorted(NEW))
def test_the_new_symbols_resolve_with_the_declared_types(name):
    from open_clip_inference import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    res, args = declared(name)
    assert len(args) == NEW[name]
    assert fn.restype == res and list(fn.argtypes) == args
    assert L.clipgpu_abi_version() == 4  # additive symbols: the ABI version stays


def test_the_prototypes_are_in_the_integration_guide():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name + "(" in text, name


@pytest.fixture()
def calls():
    """The three entry points as f(handle, nq, threshold, limit, outputs=True): every other argument valid.
    The handle of the value refusals is the address of zeroed memory: those refusals come before the handle
    is looked at, so it is never read."""
    from open_clip_inference import _lib
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data

    def device(h, nq, thr, cap, out=True):
        o = p if out else None
        return L.clipgpu_index_range_search_device(h, p, nq, thr, 1.0, 0.0, None, cap, o, p, p, p, None)

    def host(h, nq, thr, cap, out=True):
        o = p if out else None
        return L.clipgpu_index_range_search(h, p, nq, thr, 1.0, 0.0, None, cap, p, p, o, p)

    def join(h, nq, thr, cap, out=True):  # no nq
        o = p if out else None
        return L.clipgpu_index_self_join(h, thr, 1.0, 0.0, None, cap, p, o, p, p)

    fake = np.zeros(4096, np.uint8)
    return L, {"device": device, "host": host, "join": join}, fake.ctypes.data, fake


def test_the_refusals_come_before_any_device_call(calls):
    L, fns, h, _keep = calls

    def refused(rc, text):
        assert rc == INVALID
        assert text in L.clipgpu_last_error(), L.clipgpu_last_error()

    for name, f in fns.items():
        refused(f(None, 1, 0.5, 10), b"NULL")
        refused(f(h, 1, 0.5, 10, out=False), b"NULL")
        refused(f(h, 1, NAN, 10), b"threshold must not be NaN")
        for cap in (0, -1, (1 << 28) + 1, 1 << 40):
            refused(f(h, 1, 0.5, cap), b"must be in 1..268435456")
        what = {"device": b"capacity", "host": b"max_results", "join": b"max_pairs"}[name]
        refused(f(h, 1, 0.5, 0), what)
        if name != "join":
            for nq in (0, -3):
                refused(f(h, nq, 0.5, 10), b"Empty batch")
            refused(f(h, 1 << 31, 0.5, 10), b"too many queries")
            # the order of the refusals: the batch before the threshold before the capacity
            refused(f(h, 0, NAN, 0), b"Empty batch")
        refused(f(h, 1, NAN, 0), b"threshold")
        for thr in (INF, -INF):  # infinite thresholds are values like any other: the next refusal answers
            refused(f(h, 1, thr, 0), b"must be in 1..")


def test_the_python_layer_checks_its_arguments_before_any_native_call(monkeypatch):
    """The stand-in index has no handle, and the library loader is replaced by one that fails the test if
    it is reached."""
    from open_clip_inference import index as index_mod
    from open_clip_inference.error import ClipError

    class Stub(index_mod.EmbeddingIndex):
        def __init__(self):
            self._h = None
            self.E = 16

        def __len__(self):
            return 40

    def no_lib():
        raise AssertionError("a native call was made")

    monkeypatch.setattr(index_mod, "lib", no_lib)
    q = np.zeros((1, 16), np.float32)
    ix = Stub()
    with pytest.raises(ValueError, match="NaN"):
        ix.range_search(q, NAN)
    with pytest.raises(ValueError, match="NaN"):
        ix.duplicates(np.float32(NAN))
    with pytest.raises(ValueError, match="NaN"):
        ix.range_search_device(1, 1, NAN, 10, 1, 1, 1, 1)
    for bad in (0, -1, (1 << 28) + 1):
        with pytest.raises(ValueError, match="max_results must be in"):
            ix.range_search(q, 0.5, max_results=bad)
        with pytest.raises(ValueError, match="max_pairs must be in"):
            ix.duplicates(0.5, max_pairs=bad)
        with pytest.raises(ValueError, match="capacity must be in"):
            ix.range_search_device(1, 1, 0.5, bad, 1, 1, 1, 1)
    for bad in (2.5, "3", True):
        with pytest.raises(TypeError, match="max_results must be"):
            ix.range_search(q, 0.5, max_results=bad)
    for bad in (np.ones(40, np.uint8), np.ones(40, np.int32), np.ones((40, 1), bool)):
        with pytest.raises(TypeError, match="bool"):
            ix.range_search(q, 0.5, allow=bad)
        with pytest.raises(TypeError, match="bool"):
            ix.duplicates(0.5, allow=bad)
    for n in (0, 39, 41):
        with pytest.raises(ClipError, match="allow must have"):
            ix.range_search(q, 0.5, allow=np.ones(n, bool))
        with pytest.raises(ClipError, match="allow must have"):
            ix.duplicates(0.5, allow=np.ones(n, bool))
    with pytest.raises(ClipError, match="Shape error"):
        ix.range_search(np.zeros((1, 15), np.float32), 0.5)
    for thr in (0.5, -INF, INF):  # good ones go on to the library
        with pytest.raises(AssertionError, match="a native call was made"):
            ix.range_search(q, thr, allow=np.ones(40, bool))
        with pytest.raises(AssertionError, match="a native call was made"):
            ix.duplicates(thr, allow=np.ones(40, bool))


def test_the_overflow_error_carries_the_needed_size():
    from open_clip_inference.error import ClipError, InferenceError, ResultOverflow
    e = ResultOverflow("result overflow: 12 results, max_results is 11", 12)
    assert isinstance(e, InferenceError) and isinstance(e, ClipError) and e.needed == 12


L35 = np.array([[1.0, 2.0, np.nan, 2.0, 3.0],
                [-np.inf, 0.0, -0.0, np.inf, 2.0],
                [np.nan, np.nan, 1.5, 1.9999999, 2.0000002]], np.float32)


def test_the_range_oracle_on_a_hand_written_matrix():
    # a tie at the threshold (row 0: columns 1 and 3 both score exactly 2), a NaN, and >= against >
    lims, idx, score = cases.range_oracle(L35, 2.0)
    assert lims.tolist() == [0, 3, 5, 6]
    assert idx.tolist() == [4, 1, 3, 3, 4, 4]
    assert score.tolist() == [3.0, 2.0, 2.0, np.inf, 2.0, np.float32(2.0000002)]
    assert lims.dtype == np.int64 and idx.dtype == np.int64 and score.dtype == np.float32
    # the next f32 above the threshold drops exactly the ties
    lims, idx, _ = cases.range_oracle(L35, np.nextafter(np.float32(2.0), np.float32(np.inf)))
    assert lims.tolist() == [0, 1, 2, 3] and idx.tolist() == [4, 3, 4]
    # -inf takes everything but the NaNs; +0.0 and -0.0 tie and come out by ascending column
    lims, idx, _ = cases.range_oracle(L35, -np.inf)
    assert lims.tolist() == [0, 4, 9, 12]
    assert idx.tolist() == [4, 1, 3, 0, 3, 4, 1, 2, 0, 4, 3, 2]
    # live & allow
    ok = np.array([True, False, True, True, False])
    lims, idx, _ = cases.range_oracle(L35, 2.0, ok)
    assert lims.tolist() == [0, 1, 2, 2] and idx.tolist() == [3, 3]
    # nothing
    lims, idx, score = cases.range_oracle(L35[:2, :3], np.inf)
    assert lims.tolist() == [0, 0, 0] and idx.size == 0 and score.size == 0


def test_the_join_oracle_on_a_hand_written_matrix():
    S = np.array([[1.0, 0.9, np.nan, 0.5],
                  [0.9, 1.0, 0.9, 0.95],
                  [np.nan, 0.9, 1.0, 0.2],
                  [0.5, 0.95, 0.2, 1.0]], np.float32)
    pairs, score = cases.join_oracle(S, np.float32(0.9))
    assert pairs.tolist() == [[0, 1], [1, 2], [1, 3]]  # no (i, i), no (j, i), the NaN never passes
    assert np.array_equal(score, np.array([0.9, 0.9, 0.95], np.float32))
    pairs, _ = cases.join_oracle(S, np.nextafter(np.float32(0.9), np.float32(1)))
    assert pairs.tolist() == [[1, 3]]
    pairs, _ = cases.join_oracle(S, np.float32(0.9), np.array([True, True, False, True]))
    assert pairs.tolist() == [[0, 1], [1, 3]]
    pairs, score = cases.join_oracle(S[:1, :1], -np.inf)
    assert pairs.shape == (0, 2) and score.size == 0
