"""The host side of the embedding index's probability search (no GPU): the two new symbols of libclipgpu.so
with their declared argument types, the refusals that need no device, the argument checks that
EmbeddingIndex.search_probs makes before it reaches the library, and the bound B of
tests/index_probs_cases.py itself: a numpy-f32 model of the kernels' (m, s) accumulation stays within B of
float64, and three mistakes the GPU tests are there to catch each exceed it."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import index_probs_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C = {"clipgpu_index*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p,
     "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const uint32_t*": ctypes.c_void_p,
     "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}
NEW = ["clipgpu_index_search_probs", "clipgpu_index_search_probs_device"]


def declared(name):
    """(return type, argument types) of `name` as include/clipgpu.h declares it, as ctypes types."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipgpu.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    args = [C[" ".join(a.split()[:-1])] for a in m.group(2).split(",")]  # drop the parameters' names
    return C[m.group(1)], args


@pytest.mark.parametrize("name", NEW)
def test_the_new_symbols_resolve_with_the_declared_types(name):
    from open_clip_inference import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    res, args = declared(name)
    assert len(args) == (13 if name.endswith("_device") else 12)
    assert fn.restype == res and list(fn.argtypes) == args
    assert L.clipgpu_abi_version() == 4  # additive symbols: the ABI version stays


def test_null_handles_and_bad_activations_are_refused_without_a_device():
    from open_clip_inference import _lib
    L = _lib.lib()
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data
    for act in (0, 1):
        assert L.clipgpu_index_search_probs(None, p, 1, 1, 1.0, 0.0, act, None, p, p, p, None) != 0
        assert b"NULL" in L.clipgpu_last_error()
        assert L.clipgpu_index_search_probs_device(None, p, 1, 1, 1.0, 0.0, act, None, p, p, p, None, None) != 0
        assert b"NULL" in L.clipgpu_last_error()
    for act in (2, 3, -1, 1 << 20):  # CLIPGPU_SIM_LOGITS and unknown values: before the handle is looked at
        assert L.clipgpu_index_search_probs(None, p, 1, 1, 1.0, 0.0, act, None, p, p, p, None) != 0
        assert b"activation" in L.clipgpu_last_error()
        assert L.clipgpu_index_search_probs_device(None, p, 1, 1, 1.0, 0.0, act, None, p, p, p, None, None) != 0
        assert b"activation" in L.clipgpu_last_error()


def test_search_probs_checks_its_arguments_before_any_native_call(monkeypatch):
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
    for act in ("logits", "SOFTMAX", "", None, 0):
        with pytest.raises(ValueError, match="activation"):
            ix.search_probs(q, 3, activation=act)
        with pytest.raises(ValueError, match="activation"):
            ix.search_probs_device(1, 1, 3, 1, 1, 1, activation=act)
    for k in (0, -1, 129):
        with pytest.raises(ValueError, match="k must be"):
            ix.search_probs(q, k)
        with pytest.raises(ValueError, match="k must be"):
            ix.search_probs_device(1, 1, k, 1, 1, 1)
    for k in (2.5, "3", True):
        with pytest.raises(TypeError, match="k must be"):
            ix.search_probs(q, k)
    for bad in (np.ones(40, np.uint8), np.ones(40, np.int32), np.ones((40, 1), bool)):
        with pytest.raises(TypeError, match="bool"):
            ix.search_probs(q, 3, allow=bad)
    for n in (0, 39, 41):
        with pytest.raises(ClipError, match="allow must have"):
            ix.search_probs(q, 3, allow=np.ones(n, bool))
    with pytest.raises(ClipError, match="Shape error"):
        ix.search_probs(np.zeros((1, 15), np.float32), 3)
    for act in ("softmax", "sigmoid"):  # good ones go on to the library
        with pytest.raises(AssertionError, match="a native call was made"):
            ix.search_probs(q, 3, activation=act, allow=np.ones(40, bool), return_norm=True)


def test_the_bound_is_below_the_cap_at_every_test_shape():
    for N in (1, 50, 130):
        B, BS = cases.bound_for(N, 2.0)
        assert BS < B < 2.0 ** -16
        assert np.exp(-2.0) / N >= 4 * cases.CAP  # one column miscounted moves every probability this far
    for R in (2.0, 200.0):
        assert cases.bound_for(1037, R)[0] <= cases.CAP
    assert cases.bound_for(1037, 200.0)[0] < 4.4e-5
    # a million rows at scale 100 under the engine's cuts (256 spans of 4096 columns; 2048 of 512)
    assert max(cases.bound(256, 256, 200.0), cases.bound(32, 2048, 200.0)) <= cases.CAP


SPANS = (64, 64, 2)


def model_logits(scale):
    g, q = cases.rows(130)
    L = (q[:5].astype(np.float64) @ g.astype(np.float64).T * scale).astype(np.float32)
    if scale == 1.0:
        assert np.abs(L).max() <= 1.0
    return L


@pytest.mark.parametrize("scale", [1.0, 100.0])
def test_the_model_of_the_accumulation_stays_within_the_bound(scale):
    L = model_logits(scale)
    _, M, S, R = cases.oracle(L)
    BS = cases.bound_sum(4, 3, R)  # 64 columns: four per lane; three spans
    assert BS <= cases.bound_for(130, R)[1]
    for i in range(len(L)):
        m, s = cases.model(L[i], SPANS)
        assert np.float32(m).view(np.uint32) == M[i].view(np.uint32)
        assert abs(float(s) - S[i]) <= BS * S[i], (i, float(s), S[i])


@pytest.mark.parametrize("mutant", cases.MUTANTS)
def test_a_mutant_exceeds_the_bound(mutant):
    """On the scale-1 input every logit lies in [-1, 1]: a column counted twice, a dropped span or an
    omitted rescale moves S by far more than B_S, evaluated as the GPU tests evaluate it (bound_for)."""
    L = model_logits(1.0)
    _, M, S, R = cases.oracle(L)
    BS = cases.bound_for(130, R)[1]
    for i in range(len(L)):
        m, s = cases.model(L[i], SPANS, mutant)
        assert abs(float(s) - S[i]) > BS * S[i], (mutant, i)
