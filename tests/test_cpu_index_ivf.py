"""The host side of the embedding index's inverted lists and probed search (no GPU): the oracles of
tests/index_ivf_cases.py against brute force, every mutant of them caught by the assertions that
tests/test_gpu_index_ivf.py makes on the very inputs it uses, the new symbols with their declared types, and the
refusals made before any device or native call."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import index_ivf_cases as cases
from tests.index_cases import assert_same, pattern, tied_gallery

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
CT = {"clipgpu_index*": P, "const clipgpu_index*": P, "const int64_t*": P, "int64_t*": P, "const float*": P,
      "float*": P, "const uint32_t*": P, "void*": P, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
      "int": ctypes.c_int}
NEW = {"clipgpu_index_partition": 4, "clipgpu_index_partition_lists": 1, "clipgpu_index_get_lists": 3,
       "clipgpu_index_drop_partition": 1, "clipgpu_index_search_probed": 11,
       "clipgpu_index_search_probed_device": 12}
INVALID = 1  # CLIPGPU_ERR_INVALID
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


# ---- the oracles against brute force --------------------------------------------------------------------
def test_lists_oracle_on_a_hand_written_label_vector():
    labels = np.array([2, 0, -1, 2, 1, 0, -1, 2, 4])
    offsets, ids = cases.lists_oracle(labels, 6)
    assert offsets.tolist() == [0, 2, 3, 6, 6, 7, 7]  # list 3 and list 5 are empty
    assert ids.tolist() == [1, 5, 4, 0, 3, 7, 8]      # the dead rows 2 and 6 are in no list
    brute = [[j for j in range(len(labels)) if labels[j] == c] for c in range(6)]
    assert [ids[a:b].tolist() for a, b in zip(offsets[:-1], offsets[1:])] == brute
    assert cases.lists_oracle(labels, 6, descending=True)[1].tolist() == [5, 1, 4, 7, 3, 0, 8]


def test_probes_oracle_on_a_hand_written_matrix():
    Lc = np.array([[1.0, 3.0, 3.0, NAN], [0.0, -0.0, -INF, 0.5]], np.float32)
    assert cases.probes_oracle(Lc, 2).tolist() == [[1, 2], [3, 0]]  # ties (and -0.0 == +0.0) to the lower centroid
    assert cases.probes_oracle(Lc, 2, tie_high=True).tolist() == [[2, 1], [3, 1]]
    assert cases.probes_oracle(Lc, 6).tolist() == [[1, 2, 0, 3, -1, -1], [3, 0, 1, 2, -1, -1]]  # a NaN below -inf


@pytest.mark.parametrize("E,N,C", [(16, 300, 17), (80, 300, 17), (512, 300, 17), (16, 1, 17), (16, 17, 17),
                                   (16, 1200, 17), (16, 300, 1), (16, 300, 3), (16, 300, 65)])
def test_the_planted_inputs_have_the_prescribed_lists(E, N, C):
    """cases.planted asserts the f64 gap itself; here: the lengths are the prescribed ones."""
    rows, cen, label = cases.planted(E, N, C)
    assert np.bincount(label, minlength=C).tolist() == cases.lengths_for(N, C)
    assert sum(cases.lengths_for(N, C)) == N
    if N >= 300 and C >= 7:
        assert set(cases.SEAMS) <= set(cases.lengths_for(N, C))


def test_the_probed_oracle_is_the_filtered_oracle_of_the_probed_rows():
    rows, cen, label = cases.planted(16, 300, 17)
    q = cases.queries(16, 5)
    L, Lc = cases.logits64(q, rows, 100.0, 0.5), cases.logits64(q, cen)
    ok = pattern(300)
    for nprobe in (1, 2, 17, 22):
        probes = cases.probes_oracle(Lc, nprobe)
        for k in (1, 10, 128):
            assert_same(cases.probed_oracle(L, label, probes, ok, k), cases.brute_probed(L, label, probes, ok, k))
    full = cases.probed_oracle(L, label, cases.probes_oracle(Lc, 17), np.ones(300, bool), 10)
    order = np.argsort(-L, axis=1, kind="stable")[:, :10]
    assert np.array_equal(full[0], order)  # every list probed: the plain search


# ---- every assertion of the GPU file catches the matching mutant ----------------------------------------
def test_the_position_key_mutant_is_caught_by_tied_rows_in_several_lists():
    """Equal scores across lists: the row id decides, not the place in the probed lists."""
    rng = np.random.default_rng(3)
    base, g, _ = tied_gallery(rng, 300, 64)
    label = (np.arange(300) * 7) % 5  # copies of one row spread over five lists
    q = base[:3]
    L = cases.logits64(q, g, 100.0)
    probes = np.array([[4, 0, 2], [3, 1, 0], [2, 4, 1]])
    ok = np.ones(300, bool)
    good = cases.probed_oracle(L, label, probes, ok, 10)
    assert differs(good, cases.probed_oracle(L, label, probes, ok, 10, by_position=True))
    assert (np.diff(good[0][:, :5], axis=1) > 0).all()  # the tied best rows come out by ascending id


def test_the_partial_tile_and_last_probe_mutants_are_caught_by_the_planted_lists():
    rows, cen, label = cases.planted(16, 300, 17)
    q = cases.queries(16, 5)
    L, ok = cases.logits64(q, rows, 100.0), np.ones(300, bool)
    for nprobe in (1, 2, 17):
        probes = cases.probes_oracle(cases.logits64(q, cen), nprobe)
        good = cases.probed_oracle(L, label, probes, ok, 10)
        assert differs(good, cases.probed_oracle(L, label, probes, ok, 10, drop_partial_tile=True)), nprobe
        if nprobe < 17:  # the seventeenth-best list of a query holds none of its ten best rows
            assert differs(good, cases.probed_oracle(L, label, probes, ok, 10, drop_last_probe=True)), nprobe


def test_the_dead_row_mutant_is_caught_by_a_removed_best_row():
    rows, cen, label = cases.planted(16, 300, 17)
    q = cases.queries(16, 5)
    L = cases.logits64(q, rows, 100.0)
    probes = cases.probes_oracle(cases.logits64(q, cen), 2)
    best = cases.probed_oracle(L, label, probes, np.ones(300, bool), 1)[0][:, 0]
    ok = np.ones(300, bool)
    ok[best[best >= 0]] = False
    good = cases.probed_oracle(L, label, probes, ok, 10)
    assert differs(good, cases.probed_oracle(L, label, probes, ok, 10, count_dead=True))
    assert not np.isin(good[0], best[best >= 0]).any()


def test_the_centroid_tie_mutant_is_caught_by_duplicate_centroids():
    rows, cen, label = cases.planted(16, 300, 17)
    cen2 = np.concatenate([cen, cen[:4]])  # centroids 17 .. 20 are copies of 0 .. 3: nobody's label, tied scores
    Lc = cases.logits64(cases.queries(16, 5), cen2)
    assert not np.array_equal(cases.probes_oracle(Lc, 2), cases.probes_oracle(Lc, 2, tie_high=True))


def test_the_descending_ids_mutant_is_caught_by_any_list_of_two():
    _, _, label = cases.planted(16, 300, 17)
    good, bad = cases.lists_oracle(label, 17), cases.lists_oracle(label, 17, descending=True)
    assert np.array_equal(good[0], bad[0]) and not np.array_equal(good[1], bad[1])
    assert all((np.diff(good[1][a:b]) > 0).all() for a, b in zip(good[0][:-1], good[0][1:]))


# ---- the C ABI and the Python layer ---------------------------------------------------------------------
def declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipgpu.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return CT[m.group(1)], [CT[" ".join(a.split()[:-1])] for a in m.group(2).split(",")]


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


def test_the_hooks_take_zero_and_refuse_negatives():
    from open_clip_inference import _lib
    L = _lib.lib()
    for fn in (L.clipgpu_test_probe_parts, L.clipgpu_test_probe_chunk):
        assert fn(3) == 0 and fn(0) == 0
        assert fn(-1) == INVALID


def test_the_refusals_come_before_any_device_call():
    """The handle of the value refusals is the address of zeroed memory: they come before it is looked at."""
    from open_clip_inference import _lib
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p, h = buf.ctypes.data, np.zeros(4096, np.uint8).ctypes.data

    def refused(rc, text):
        assert rc == INVALID
        assert text in L.clipgpu_last_error(), L.clipgpu_last_error()

    refused(L.clipgpu_index_partition(None, p, 1, None), b"NULL")
    refused(L.clipgpu_index_partition(h, None, 1, None), b"NULL")
    for C in (0, -1, 65537, 1 << 40):
        refused(L.clipgpu_index_partition(h, p, C, None), b"centroids must be in 1..65536")
    refused(L.clipgpu_index_get_lists(None, p, p), b"NULL")
    refused(L.clipgpu_index_get_lists(h, None, p), b"NULL")
    refused(L.clipgpu_index_drop_partition(None), b"NULL")
    assert L.clipgpu_index_partition_lists(None) == 0
    for fn, tail in ((L.clipgpu_index_search_probed, (p,)), (L.clipgpu_index_search_probed_device, (p, None))):
        refused(fn(None, p, 1, 1, 1, 1.0, 0.0, None, p, p, *tail), b"NULL")
        refused(fn(h, None, 1, 1, 1, 1.0, 0.0, None, p, p, *tail), b"NULL")
        refused(fn(h, p, 1, 1, 1, 1.0, 0.0, None, None, p, *tail), b"NULL")
        refused(fn(h, p, 0, 1, 1, 1.0, 0.0, None, p, p, *tail), b"Empty batch")
        for k in (0, 129):
            refused(fn(h, p, 1, k, 1, 1.0, 0.0, None, p, p, *tail), b"k must be in 1..128")
        for nprobe in (0, 129, -3):
            refused(fn(h, p, 1, 1, nprobe, 1.0, 0.0, None, p, p, *tail), b"nprobe must be in 1..128")


def test_the_python_layer_checks_its_arguments_before_any_native_call(monkeypatch):
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
    ix, c, q = Stub(), np.zeros((3, 16), np.float32), np.zeros((2, 16), np.float32)
    with pytest.raises(ClipError, match="Shape error"):
        ix.partition(np.zeros((3, 15), np.float32))
    with pytest.raises(ValueError, match="centroids must be in 1..65536"):
        ix.partition(np.zeros((0, 16), np.float32))
    with pytest.raises(ValueError, match="centroids must be in 1..65536"):
        ix.partition(np.zeros((65537, 16), np.float32))
    for bad in (0, 129, -1):
        with pytest.raises(ValueError, match="nprobe must be in 1..128"):
            ix.search_probed(q, 5, bad)
        with pytest.raises(ValueError, match="k must be in 1..128"):
            ix.search_probed(q, bad, 2)
        with pytest.raises(ValueError, match="nprobe must be in 1..128"):
            ix.search_probed_device(1, 2, 5, bad, 1, 1)
    for bad in (2.0, "3", True):
        with pytest.raises(TypeError, match="nprobe must be an integer"):
            ix.search_probed(q, 5, bad)
        with pytest.raises(TypeError, match="k must be an integer"):
            ix.search_probed(q, bad, 2)
    with pytest.raises(TypeError, match="bool"):
        ix.search_probed(q, 5, 2, allow=np.ones(40, np.uint8))
    with pytest.raises(ClipError, match="allow must have"):
        ix.search_probed(q, 5, 2, allow=np.ones(39, bool))
    with pytest.raises(ClipError, match="Shape error"):
        ix.search_probed(np.zeros((2, 15), np.float32), 5, 2)
    with pytest.raises(ValueError, match="n_clusters must be in"):
        ix.partition_kmeans(0)
    for call in (lambda: ix.partition(c), lambda: ix.search_probed(q, 5, 2), lambda: ix.drop_partition(),
                 lambda: ix.n_lists):
        with pytest.raises(AssertionError, match="a native call was made"):  # good ones go on to the library
            call()
