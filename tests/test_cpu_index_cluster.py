"""The host side of the embedding index's assignment and k-means (no GPU): the oracles of
tests/index_cluster_cases.py on hand-written inputs, every mutant of them caught by the assertions that
tests/test_gpu_index_cluster.py makes on the very inputs it uses, the bound on the integer sums, the new symbols
with their declared types, and the refusals made before any device or native call."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import index_cluster_cases as cases
from tests.index_cases import pattern, unit_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
CT = {"clipgpu_index*": P, "const int64_t*": P, "int64_t*": P, "int32_t*": P, "const float*": P, "float*": P,
      "const uint32_t*": P, "void*": P, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}
NEW = {"clipgpu_index_assign_device": 9, "clipgpu_index_assign": 8, "clipgpu_index_kmeans": 10,
       "clipgpu_index_get_rows_at": 4}
INVALID = 1  # CLIPGPU_ERR_INVALID
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def same(a, b):
    """Every field of two lloyd results is equal, as assert_kmeans compares them."""
    return all(np.array_equal(np.asarray(a[k]).view(np.uint32) if np.asarray(a[k]).dtype == np.float32 else a[k],
                              np.asarray(b[k]).view(np.uint32) if np.asarray(b[k]).dtype == np.float32 else b[k])
               for k in a)


# ---- assign_oracle --------------------------------------------------------------------------------------
def test_assign_oracle_on_a_hand_written_matrix():
    L = np.array([[1.0, 0.0, NAN, -INF, 2.0],
                  [1.0, -0.0, -INF, NAN, 3.0],
                  [0.5, -1.0, NAN, NAN, 3.0]], np.float32)
    labels, scores = cases.assign_oracle(L)
    assert labels.tolist() == [0, 0, 1, 0, 1]  # ties (and -0.0 == +0.0) to the lower index; a NaN below -inf
    assert scores[:2].view(np.uint32).tolist() == [0x3F800000, 0] and scores[2] == -INF and scores[3] == -INF
    ok = np.array([True, False, True, True, False])
    labels, scores = cases.assign_oracle(L, ok)
    assert labels.tolist() == [0, -1, 1, 0, -1] and scores[1] == -INF and scores[4] == -INF
    # all NaN: the lower index, and its NaN
    labels, scores = cases.assign_oracle(np.full((3, 2), NAN))
    assert labels.tolist() == [0, 0] and np.isnan(scores).all()
    # the mutants differ exactly where they should
    assert cases.assign_oracle(L, tie_high=True)[0].tolist() == [1, 1, 1, 0, 2]
    assert cases.assign_oracle(L, ok, count_dead=True)[0].tolist() == [0, 0, 1, 0, 1]


def test_the_key_of_the_oracle_is_the_library_key():
    from open_clip_inference import _lib
    vals = np.array([0.0, -0.0, 1.5, -1.5, INF, -INF, NAN, 1e-45, -1e-45], np.float32)
    for c in (0, 3, 70, 65535):
        for v, m in zip(vals, cases.mono(vals)):
            k = ctypes.c_uint64()
            _lib.check(_lib.lib().clipgpu_test_topk_key(float(v), c, ctypes.byref(k)))
            assert k.value == (int(m) << 32) | (~c & 0xFFFFFFFF), (v, c)


# ---- the update -----------------------------------------------------------------------------------------
def test_the_shift_rule():
    assert cases.shift_of(np.ones((1 << 10, 4), np.float32)) == 62 - 1 - 11
    assert cases.shift_of(np.zeros((5, 4), np.float32)) == 62 - 0 - 3
    assert cases.shift_of(np.full((7, 4), 0.75, np.float32)) == 62 - 0 - 3
    assert cases.shift_of(np.full((8, 4), -3.0, np.float32)) == 62 - 2 - 4
    rows = np.ones((6, 4), np.float32)
    rows[4, 2] = INF
    rows[5, 0] = NAN
    with pytest.raises(ValueError, match="row 4 "):
        cases.shift_of(rows)
    ok = np.array([True, True, True, True, False, True])
    with pytest.raises(ValueError, match="row 5 "):
        cases.shift_of(rows, ok)
    assert cases.shift_of(rows, ok & (np.arange(6) < 4)) == 62 - 1 - 3  # non-finite rows that are not counted


@pytest.mark.parametrize("m", [1.0, float(np.nextafter(np.float32(2.0), np.float32(0.0)))])
def test_the_sums_stay_below_2_to_the_62_at_a_million_rows(m):
    n = 1 << 20
    rows = np.full((n, 1), m, np.float32)
    s = cases.shift_of(rows)
    assert s == 40  # e = 1, b = 21
    S = cases.fixed_sums(rows, np.zeros(n, np.int64), 1, s)
    exact = n * int(np.rint(np.ldexp(np.float64(np.float32(m)), s)))  # Python integers: no wrap
    assert int(S[0, 0]) == exact and 0 < exact < 1 << 62
    assert abs(int(cases.fixed_sums(-rows, np.zeros(n, np.int64), 1, s)[0, 0])) < 1 << 62


def test_fixed_sums_round_to_nearest_even():
    rows = np.array([[0.5, 1.5, 2.5, -0.5, -1.5, 0.75, -0.75, 1.25]], np.float32)
    lab = np.zeros(1, np.int64)
    assert cases.fixed_sums(rows, lab, 1, 0).tolist() == [[0, 2, 2, 0, -2, 1, -1, 1]]
    assert cases.fixed_sums(rows, lab, 1, 0, truncate=True).tolist() == [[0, 1, 2, 0, -1, 0, 0, 1]]
    assert cases.fixed_sums(rows, lab, 1, 2).tolist() == [[2, 6, 10, -2, -6, 3, -3, 5]]  # exact after the scaling
    assert cases.fixed_sums(rows, np.array([-1]), 2, 0).tolist() == [[0] * 8] * 2  # an unlabelled row adds nothing


def test_finalise_on_a_hand_written_case():
    S = np.array([[3, 4], [0, 0], [5, -5], [7, 0]], np.int64)
    prev = np.arange(8, dtype=np.float32).reshape(4, 2)
    out = cases.finalise(S, np.array([2, 0, 2, 0]), prev)
    assert out[0].tolist() == [np.float32(0.6), np.float32(0.8)]
    assert out[1].tolist() == [2.0, 3.0] and out[3].tolist() == [6.0, 7.0]  # empty: kept, whatever S says
    assert out[2].tolist() == [np.float32(np.sqrt(0.5)), -np.float32(np.sqrt(0.5))]
    assert cases.finalise(S, np.array([2, 2, 2, 2]), prev)[1].tolist() == [2.0, 3.0]  # members that cancel: kept
    assert cases.finalise(S, np.array([2, 0, 2, 0]), prev, zero_empty=True)[1].tolist() == [0.0, 0.0]


# ---- every mutant is caught on the inputs of the GPU tests ----------------------------------------------
def test_lloyd_recovers_the_planted_blobs():
    rows, init, blob = cases.blobs()
    r = cases.lloyd(rows, init, 25)
    assert np.array_equal(r["labels"], blob) and r["counts"].tolist() == [125] * 8
    assert r["moved"][0] == 1000 and r["moved"][-1] == 0 and r["iters"] == len(r["moved"]) >= 2
    again = cases.lloyd(rows, r["centroids"], 25)  # a converged result is a fixed point
    assert same(again, dict(r, moved=np.array([1000, 0]), iters=2))


def test_the_tie_mutant_is_caught_by_duplicated_centroids():
    rows, cen = cases.tie_case()
    L = cases.logits64(cen, rows)
    good, bad = cases.assign_oracle(L), cases.assign_oracle(L, tie_high=True)
    assert good[0][10] == 3 and good[0][20] == 64 and not np.isin(good[0], (70, 129)).any()
    assert bad[0][10] == 70 and bad[0][20] == 129


def test_the_dead_row_mutant_is_caught_by_the_mask_cases():
    rows, init, _ = cases.blobs()
    ok = pattern(1000)
    good, bad = cases.assign_oracle(cases.logits64(init, rows), ok), cases.assign_oracle(
        cases.logits64(init, rows), ok, count_dead=True)
    assert (good[0][~ok] == -1).all() and (bad[0] >= 0).all()
    assert not same(cases.lloyd(rows, init, 3, ok), cases.lloyd(rows, init, 3, ok, count_dead=True))


def test_the_rounding_and_shift_mutants_are_caught_on_the_wide_rows():
    rows, init = cases.wide_rows()
    labels, _ = cases.assign_oracle(cases.logits64(init, rows))
    S = cases.fixed_sums(rows, labels, 4, 7)
    assert not np.array_equal(S, cases.fixed_sums(rows, labels, 4, 7, truncate=True))
    # half away from zero instead of to even differs in row 1 alone: the sums see that too
    away = np.ldexp(rows.astype(np.float64), 7)
    away = (np.sign(away) * np.floor(np.abs(away) + 0.5)).astype(np.int64)
    assert (away[1] != np.rint(np.ldexp(rows[1].astype(np.float64), 7))).any()
    assert cases.shift_of(rows, one_small=True) == 6
    assert not np.array_equal(S, cases.fixed_sums(rows, labels, 4, 6))
    good = cases.lloyd(rows, init, 1)
    assert not same(good, cases.lloyd(rows, init, 1, truncate=True))  # the centroids' bits see the rounding


def test_the_empty_cluster_mutant_is_caught_by_a_centroid_at_minus_the_mean():
    rows, start = cases.biased_rows()
    good, bad = cases.lloyd(rows, start, 4), cases.lloyd(rows, start, 4, zero_empty=True)
    assert good["counts"][5] == 0 and np.array_equal(good["centroids"][5].view(np.uint32), start[5].view(np.uint32))
    assert not bad["centroids"][5].any()


def test_the_stale_label_mutant_is_caught_by_an_unconverged_run():
    rows, init = cases.generic_rows()
    good, bad = cases.lloyd(rows, init, 2), cases.lloyd(rows, init, 2, stale_labels=True)
    assert good["iters"] == 2 and good["moved"][-1] > 0  # stopped by max_iter
    now = cases.assign_oracle(cases.logits64(good["centroids"], rows))
    assert np.array_equal(good["labels"], now[0]) and not np.array_equal(bad["labels"], now[0])


def test_a_permuted_gallery_gives_the_same_centroids():
    rows, init = cases.generic_rows()
    perm = np.random.default_rng(1).permutation(len(rows))
    a, b = cases.lloyd(rows, init, 6), cases.lloyd(rows[perm], init, 6)
    assert np.array_equal(a["centroids"].view(np.uint32), b["centroids"].view(np.uint32))
    assert np.array_equal(a["labels"][perm], b["labels"]) and np.array_equal(a["moved"], b["moved"])


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


def test_the_refusals_come_before_any_device_call():
    """The handle of the value refusals is the address of zeroed memory: they come before it is looked at."""
    from open_clip_inference import _lib
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p, h = buf.ctypes.data, np.zeros(4096, np.uint8).ctypes.data

    def refused(rc, text):
        assert rc == INVALID
        assert text in L.clipgpu_last_error(), L.clipgpu_last_error()

    refused(L.clipgpu_index_assign(None, p, 1, 1.0, 0.0, None, p, p), b"NULL")
    refused(L.clipgpu_index_assign(h, None, 1, 1.0, 0.0, None, p, p), b"NULL")
    refused(L.clipgpu_index_assign(h, p, 1, 1.0, 0.0, None, None, p), b"NULL")
    refused(L.clipgpu_index_assign_device(h, p, 1, 1.0, 0.0, None, p, None, None), b"NULL")
    refused(L.clipgpu_index_kmeans(h, 1, p, 5, None, p, p, p, p, None), b"NULL")
    refused(L.clipgpu_index_kmeans(None, 1, p, 5, None, p, p, p, p, p), b"NULL")
    for C in (0, -1, 65537, 1 << 40):
        refused(L.clipgpu_index_assign(h, p, C, 1.0, 0.0, None, p, p), b"centroids must be in 1..65536")
        refused(L.clipgpu_index_assign_device(h, p, C, 1.0, 0.0, None, p, p, None), b"centroids must be in 1..65536")
        refused(L.clipgpu_index_kmeans(h, C, p, 5, None, p, p, p, p, p), b"centroids must be in 1..65536")
    for it in (0, -2):
        refused(L.clipgpu_index_kmeans(h, 1, p, it, None, p, p, p, p, p), b"max_iter must be at least 1")
    refused(L.clipgpu_index_get_rows_at(None, p, 1, p), b"NULL")
    refused(L.clipgpu_index_get_rows_at(h, None, 1, p), b"NULL")
    refused(L.clipgpu_index_get_rows_at(h, p, -1, p), b"negative")


def test_the_python_layer_checks_its_arguments_before_any_native_call(monkeypatch):
    from open_clip_inference import index as index_mod
    from open_clip_inference.error import ClipError

    class Stub(index_mod.EmbeddingIndex):
        def __init__(self):
            self._h = None
            self.E = 16

        def __len__(self):
            return 40

        def is_live(self):
            return np.arange(40) % 2 == 0  # 20 live rows

    def no_lib():
        raise AssertionError("a native call was made")

    monkeypatch.setattr(index_mod, "lib", no_lib)
    ix, c = Stub(), np.zeros((3, 16), np.float32)
    with pytest.raises(ClipError, match="Shape error"):
        ix.assign(np.zeros((3, 15), np.float32))
    with pytest.raises(ValueError, match="centroids must be in 1..65536"):
        ix.assign(np.zeros((0, 16), np.float32))
    with pytest.raises(ValueError, match="centroids must be in 1..65536"):
        ix.kmeans(init=np.zeros((65537, 16), np.float32))
    with pytest.raises(TypeError, match="bool"):
        ix.assign(c, allow=np.ones(40, np.uint8))
    with pytest.raises(ClipError, match="allow must have"):
        ix.kmeans(init=c, allow=np.ones(39, bool))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_iter must be at least 1"):
            ix.kmeans(init=c, max_iter=bad)
    for bad in (2.5, "3", True):
        with pytest.raises(TypeError, match="max_iter must be an integer"):
            ix.kmeans(init=c, max_iter=bad)
    with pytest.raises(ValueError, match="n_clusters is required"):
        ix.kmeans()
    with pytest.raises(ValueError, match="n_clusters must be in"):
        ix.kmeans(0)
    with pytest.raises(ValueError, match="n_clusters must be in"):
        ix.kmeans(65537)
    with pytest.raises(TypeError, match="n_clusters must be an integer"):
        ix.kmeans(2.0)
    with pytest.raises(ValueError, match="n_clusters is 4 but init has 3 rows"):
        ix.kmeans(4, init=c)
    with pytest.raises(ValueError, match="n_clusters is 21 but only 20 rows are live and allowed"):
        ix.kmeans(21)
    with pytest.raises(ValueError, match="n_clusters is 11 but only 10 rows are live and allowed"):
        ix.kmeans(11, allow=np.arange(40) < 20)
    with pytest.raises(TypeError, match="integers"):
        ix.rows_at([0.5])
    for call in (lambda: ix.assign(c), lambda: ix.kmeans(init=c), lambda: ix.kmeans(20), lambda: ix.rows_at([1, 1])):
        with pytest.raises(AssertionError, match="a native call was made"):  # good ones go on to the library
            call()
