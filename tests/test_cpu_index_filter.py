"""The host side of the filtered embedding index (no GPU): the allow bitmap's layout (pack_allow: row i
at bit i & 31 of word i >> 5, numpy's packbits(bitorder="little") read as little-endian uint32), the new
symbols of libclipgpu.so with their declared argument types, and the argument checks that
EmbeddingIndex.search makes before it reaches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.index_cases import pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 31, 32, 33, 64, 65]


def reference_words(a, bitorder="little"):
    by = np.packbits(a, bitorder=bitorder)
    by = np.concatenate([by, np.zeros(-len(by) % 4, np.uint8)])
    return by.view("<u4").astype(np.uint32)


@pytest.mark.parametrize("n", LENGTHS)
def test_pack_allow_is_little_endian_packbits(n):
    from open_clip_inference.index import pack_allow
    rng = np.random.default_rng(n)
    for a in (pattern(n), np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.5):
        got = pack_allow(a)
        assert got.dtype == np.uint32 and got.shape == ((n + 31) // 32,)
        assert np.array_equal(got, reference_words(a))
        for i in range(n):  # the layout the kernels read
            assert bool((int(got[i >> 5]) >> (i & 31)) & 1) == bool(a[i])
        if n % 32:  # zero padding
            assert int(got[-1]) >> (n % 32) == 0


@pytest.mark.parametrize("n", [n for n in LENGTHS if n >= 2])
def test_a_bit_order_mutant_differs(n):
    """Packing the bits of a byte big end first (numpy's default) is a different bitmap at every length
    >= 2 for a pattern that is no palindrome, so the comparison above tells the two apart."""
    from open_clip_inference.index import pack_allow
    a = pattern(n)
    assert not np.array_equal(a[:min(n, 8)], a[:min(n, 8)][::-1])
    mutant = reference_words(a, bitorder="big")
    assert not np.array_equal(mutant, reference_words(a))
    assert not np.array_equal(pack_allow(a), mutant)


def test_pack_allow_refuses_what_is_not_a_bool_vector():
    from open_clip_inference.index import pack_allow
    for bad in (np.ones(4, np.uint8), np.ones(4, np.int64), np.ones((2, 2), bool), [1, 0, 1]):
        with pytest.raises(TypeError):
            pack_allow(bad)
    assert np.array_equal(pack_allow([True, False, True]), np.array([5], np.uint32))


C = {"clipgpu_index*": ctypes.c_void_p, "const clipgpu_index*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p,
     "int64_t*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
     "const uint32_t*": ctypes.c_void_p, "uint8_t*": ctypes.c_void_p, "void*": ctypes.c_void_p,
     "int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}
NEW = ["clipgpu_index_remove", "clipgpu_index_live", "clipgpu_index_get_live", "clipgpu_index_set_rows",
       "clipgpu_index_search_filtered", "clipgpu_index_search_filtered_device"]


def declared(name):
    """(return type, argument types) of `name` as include/clipgpu.h declares it, as ctypes types."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipgpu.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        words = a.split()
        typ = " ".join(words[:-1])  # drop the parameter's name
        args.append(C[typ])
    return C[m.group(1)], args


@pytest.mark.parametrize("name", NEW)
def test_the_new_symbols_resolve_with_the_declared_types(name):
    from open_clip_inference import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    res, args = declared(name)
    assert fn.restype == res and list(fn.argtypes) == args
    assert L.clipgpu_abi_version() == 4  # additive symbols: the ABI version stays


def test_null_handles_are_refused_without_a_device():
    from open_clip_inference import _lib
    L = _lib.lib()
    ids = np.zeros(1, np.int64)
    assert L.clipgpu_index_live(None) == 0
    assert L.clipgpu_index_remove(None, ids.ctypes.data, 1) != 0
    assert b"NULL" in L.clipgpu_last_error()
    assert L.clipgpu_index_set_rows(None, ids.ctypes.data, ids.ctypes.data, 1) != 0
    assert L.clipgpu_index_get_live(None, 0, 1, ids.ctypes.data) != 0
    assert L.clipgpu_index_search_filtered(None, None, 1, 1, 1.0, 0.0, None, None, None) != 0


def test_search_checks_allow_before_any_native_call(monkeypatch):
    """A wrong dtype or length of `allow` is refused in Python: the stand-in index has no handle, and the
    library loader is replaced by one that fails the test if it is reached."""
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
    for bad in (np.ones(40, np.uint8), np.ones(40, np.int32), np.ones(40, np.float32), np.ones((40, 1), bool)):
        with pytest.raises(TypeError, match="bool"):
            ix.search(q, 3, allow=bad)
    for n in (0, 39, 41, 64):
        with pytest.raises(ClipError, match="allow must have"):
            ix.search(q, 3, allow=np.ones(n, bool))
    with pytest.raises(AssertionError, match="a native call was made"):  # a good one goes on to the library
        ix.search(q, 3, allow=np.ones(40, bool))
