"""The host side of the embedding index's int8 codes and coded search (no GPU): the oracles of
tests/index_codes_cases.py against brute force on hand-written cases, every mutant of them caught by the
assertions that tests/test_gpu_index_codes.py makes on the very inputs it uses, the new symbols with their declared
types, and the refusals made before any device or native call."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import index_codes_cases as cases
from tests.index_cases import assert_same, pattern, tied_gallery

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
CT = {"clipgpu_index*": P, "const clipgpu_index*": P, "const int64_t*": P, "int64_t*": P, "const float*": P,
      "float*": P, "const uint32_t*": P, "int8_t*": P, "void*": P, "int64_t": ctypes.c_int64,
      "float": ctypes.c_float, "int": ctypes.c_int}
NEW = {"clipgpu_index_enable_codes": 1, "clipgpu_index_has_codes": 1, "clipgpu_index_drop_codes": 1,
       "clipgpu_index_get_codes": 5, "clipgpu_index_search_coded": 12, "clipgpu_index_search_coded_device": 13}
INVALID = 1  # CLIPGPU_ERR_INVALID
E0, N0, Q0, K0, R0 = 16, 300, 5, 10, 32  # the GPU file's defaults


def differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def setup(E=E0, N=N0, Q=Q0, scale=100.0):
    g, q = cases.gallery(E, N), cases.queries(E, Q)
    return g, q, cases.logits64(q, g, scale)


# ---- the oracles against brute force, on hand-written cases ---------------------------------------------
def test_codes_oracle_on_a_three_row_matrix():
    rows = np.zeros((3, 16), np.float32)
    rows[0, :6] = [127, 0.5, 1.5, 2.5, -2.5, 126.5]  # m = 127: inv == 1, the halves go to even
    rows[1, :4] = [2, -1, 0.5, -0.0]                  # m = 2: inv = 63.5
    rows[2, :2] = [np.nan, 1]
    codes, scale = cases.codes_oracle(rows)
    assert codes.dtype == np.int8 and scale.dtype == np.float32
    assert codes[0, :6].tolist() == [127, 0, 2, 2, -2, 126]
    assert codes[1, :4].tolist() == [127, -64, 32, 0]  # 63.5 -> 64 and 31.75 -> 32: no tie
    assert not codes[2].any() and scale[2] == 0
    assert scale[0] == 1 and scale[1] == np.float32(2) / np.float32(127)
    brute = [max(-127, min(127, round(float(np.float32(v) * (np.float32(127) / np.float32(2)))))) for v in rows[1, :4]]
    assert codes[1, :4].tolist() == brute  # Python's round is half-to-even too
    assert cases.codes_oracle(rows, half_away=True)[0][0, :6].tolist() == [127, 1, 2, 3, -3, 127]
    assert cases.codes_oracle(rows, top=128)[0][1, :4].tolist() == [127, -64, 32, 0]  # 128 cut to 127 ...
    assert cases.codes_oracle(rows, top=128)[0][0, 1:4].tolist() == [1, 2, 3]          # ... but the steps moved


def test_coarse_and_candidate_order_with_ties_and_signed_zeros():
    cq = np.array([[1, 0], [0, -1]], np.int8)
    cg = np.array([[2, 5], [2, 7], [0, 0], [-1, 3], [0, 0]], np.int8)
    sg = np.array([1, 1, 0.5, 2, 0], np.float32)
    c = cases.coarse_oracle(cq, cg, sg)
    assert c.tolist() == [[2, 2, 0, -2, 0], [-5, -7, 0, -6, 0]]
    brute = np.array([[float(sum(int(a) * int(b) for a, b in zip(qr, gr))) * float(s) for gr, s in zip(cg, sg)]
                      for qr in cq], np.float32)
    assert np.array_equal(c, brute)
    ok = np.ones(5, bool)
    cand, cs = cases.candidates_oracle(c, ok, 4)
    assert cand.tolist() == [[0, 1, 2, 4], [2, 4, 0, 3]]  # ties (and -0.0 == +0.0) to the lower row
    neg = cases.coarse_oracle(cq, cg, sg, neg=True)
    assert np.signbit(neg[0, 2]) and np.signbit(neg[1, 4])  # -(0.0): a zero of the other sign, the same key
    assert cases.candidates_oracle(neg, ok, 3)[0].tolist() == [[3, 2, 4], [1, 3, 0]]
    assert cases.candidates_oracle(c, ok, 4, tie_high=True)[0].tolist() == [[1, 0, 4, 2], [4, 2, 0, 3]]
    ok[2] = False
    assert cases.candidates_oracle(c, ok, 5)[0].tolist() == [[0, 1, 4, 3, -1], [4, 0, 3, 1, -1]]
    assert np.isneginf(cases.candidates_oracle(c, ok, 5)[1][:, 4]).all()


def test_the_list_layout_of_the_rerank():
    cand = np.array([[7, 3, 9, -1], [-1, -1, -1, -1], [1, 2, 3, 4]], np.int64)
    ids, off, lists = cases.list_layout(cand)
    assert ids.dtype == np.int32 and off.dtype == np.int32 and lists.dtype == np.int64
    assert off.tolist() == [0, 3, 4, 4, 8, 12, 12] and lists.tolist() == [0, 2, 4]
    for q in range(3):  # list 2q = the valid candidates, list 2q + 1 = the padding
        assert ids.ravel()[off[2 * q]:off[2 * q + 1]].tolist() == [c for c in cand[q] if c >= 0]
        assert off[2 * q + 2] - off[2 * q + 1] == (cand[q] < 0).sum()


def test_the_coded_oracle_is_the_filtered_oracle_of_the_candidates():
    from tests.index_cases import logits_oracle
    g, q, L = setup()
    ok = pattern(N0)
    for k, refine in ((1, 1), (10, 32), (17, 17), (128, 128)):
        want, cand, cs = cases.expect(L, g, q, ok, k, refine)
        assert ok[cand[cand >= 0]].all()
        for i in range(Q0):
            assert_same((want[0][i:i + 1], want[1][i:i + 1]), logits_oracle(L[i:i + 1], np.isin(np.arange(N0), cand[i]), k))
    small = cases.expect(L[:, :20], g[:20], q, np.ones(20, bool), 10, 32)
    assert_same(small[0], logits_oracle(L[:, :20], np.ones(20, bool), 10))  # N <= refine: the plain search


# ---- every assertion of the GPU file catches the matching mutant ----------------------------------------
@pytest.mark.parametrize("E", [16, 80, 512])
def test_the_rounding_and_clamp_mutants_are_caught_by_the_special_rows(E):
    rows = cases.special_rows(E)
    good = cases.codes_oracle(rows)
    assert not np.array_equal(good[0], cases.codes_oracle(rows, half_away=True)[0])
    assert not np.array_equal(good[0][2:4], cases.codes_oracle(rows, half_away=True)[0][2:4])  # the rows with halves
    assert not np.array_equal(good[0], cases.codes_oracle(rows, top=128)[0])
    assert good[0][2, :6].tolist() == [127, 0, 2, 2, -2, 126] and good[1][2] == 1
    for r in (0, 1, 4, 5, 6, 7):  # zeros, -0.0, a NaN, inf, -inf, 127 / m overflows
        assert not good[0][r].any() and good[1][r] == 0, r
    assert good[0][8, :3].tolist() == [127, -42, 64] and np.isfinite(good[1][8]) and good[1][8] > 1e36
    assert len(set(good[1][8:12].tolist())) == 4  # different maxima, different scales
    assert np.abs(good[0]).max() == 127 and good[0].min() == -127
    # ordinary rows too: some product lands on a half only by accident, but the clamp mutant moves every step
    g = cases.gallery(E, N0)
    assert not np.array_equal(cases.codes_oracle(g)[0], cases.codes_oracle(g, top=128)[0])


def test_the_scale_and_sign_mutants_are_caught_by_the_gallery():
    g, q, L = setup()
    cg, sg = cases.codes_oracle(g)
    cq, _ = cases.codes_oracle(q)
    ok = np.ones(N0, bool)
    assert len(set(sg.tolist())) > N0 // 2  # the rows' scales differ
    for neg in (False, True):
        good = cases.candidates_oracle(cases.coarse_oracle(cq, cg, sg, neg), ok, R0)
        assert differs(good, cases.candidates_oracle(cases.coarse_oracle(cq, cg, sg, neg, no_scale=True), ok, R0))
    good = cases.candidates_oracle(cases.coarse_oracle(cq, cg, sg, True), ok, R0)
    assert differs(good, cases.candidates_oracle(cases.coarse_oracle(cq, cg, sg, True, no_flip=True), ok, R0))
    # and the final results: a negative scale's best rows are the positive scale's worst
    Ln = cases.logits64(q, g, -100.0)
    assert differs(cases.expect(Ln, g, q, ok, K0, R0, neg=True)[0],
                   cases.coded_oracle(Ln, cases.candidates_oracle(cases.coarse_oracle(cq, cg, sg, True, no_flip=True), ok, R0)[0], K0))


def test_the_position_mutant_is_caught_by_the_tied_gallery():
    rng = np.random.default_rng(3)
    base, g, _ = tied_gallery(rng, N0, 64)
    q = base[:3]
    cg, sg = cases.codes_oracle(g)
    cq, _ = cases.codes_oracle(q)
    c = cases.coarse_oracle(cq, cg, sg)
    ok = np.ones(N0, bool)
    good = cases.candidates_oracle(c, ok, R0)
    assert differs(good, cases.candidates_oracle(c, ok, R0, tie_high=True))
    assert (np.diff(good[0][:, :20], axis=1) > 0).all()  # copies of the best row, by ascending id
    assert good[0][:, :20].max() > 128  # and from more than one 64- or 128-column span


def test_the_dead_row_mutant_is_caught_by_a_removed_best_row():
    g, q, L = setup()
    everything = np.ones(N0, bool)
    best = cases.expect(L, g, q, everything, 1, R0)[0][0][:, 0]
    ok = everything.copy()
    ok[best] = False
    good = cases.expect(L, g, q, ok, K0, R0)
    assert differs(good[0], cases.expect(L, g, q, ok, K0, R0, count_dead=True)[0])
    assert not np.isin(good[0][0], best).any() and not np.isin(good[1], best).any()


def test_the_stale_codes_mutant_is_caught_by_replaced_rows():
    g, q, L = setup()
    ok = np.ones(N0, bool)
    best = cases.expect(L, g, q, ok, 1, R0)[0][0][:, 0]
    new = g.copy()
    new[best] = -g[best]  # every query's best row becomes its worst
    stale_codes = cases.codes_oracle(g)
    assert not np.array_equal(stale_codes[0], cases.codes_oracle(new)[0])
    Lnew = cases.logits64(q, new, 100.0)
    cq, _ = cases.codes_oracle(q)
    # the candidates and their coarse scores, which the GPU file compares, show it at every refine; the re-rank is
    # exact and can hide a stale candidate behind refine - k spare ones, so the results show it at refine = k
    for refine in (R0, K0):
        good = cases.expect(Lnew, new, q, ok, K0, refine)
        stale = cases.candidates_oracle(cases.coarse_oracle(cq, *stale_codes), ok, refine)
        assert differs((good[1], good[2]), stale), refine
    assert differs(good[0], cases.coded_oracle(Lnew, stale[0], K0))


def test_the_cut_at_k_mutant_is_caught_by_the_default_shapes():
    """The coarse order is not the exact order: the k best of `refine` candidates are not the first k candidates."""
    g, q, L = setup()
    ok = np.ones(N0, bool)
    caught = []
    for k, refine in ((10, 32), (1, 16), (10, 16), (17, 128)):
        good, cut = cases.expect(L, g, q, ok, k, refine), cases.expect(L, g, q, ok, k, k)
        assert (good[1] >= 0).sum() == Q0 * min(refine, N0)  # the candidates the GPU file compares: refine of them
        assert not np.array_equal(good[1][:, :k], good[0][0]) or k == 1  # and not in the exact order
        caught.append(differs(good[0], cut[0]))
    assert any(caught), caught  # the results too, where the exact k best are not the coarse k best


@pytest.mark.parametrize("E", [16, 80, 512])
def test_the_planted_gap_exceeds_twice_the_bound(E):
    """planted_gap asserts gap > 2 B itself; here: the consequence, on the oracles."""
    rows, q, gap, B = cases.planted_gap(E, N0, Q0, K0)
    assert gap > 2 * B > 0
    L = cases.logits64(q, rows)
    from tests.index_cases import logits_oracle
    got = cases.expect(L, rows, q, np.ones(N0, bool), K0, K0)[0]
    assert_same(got, logits_oracle(L, np.ones(N0, bool), K0))


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


def test_the_stage_hook_takes_its_three_values():
    from open_clip_inference import _lib
    L = _lib.lib()
    assert L.clipgpu_test_codes_stage(1) == 0 and L.clipgpu_test_codes_stage(2) == 0 and L.clipgpu_test_codes_stage(0) == 0
    assert L.clipgpu_test_codes_stage(3) == INVALID and L.clipgpu_test_codes_stage(-1) == INVALID


def test_the_refusals_come_before_any_device_call():
    """The handle of the value refusals is the address of zeroed memory: an index without codes."""
    from open_clip_inference import _lib
    L = _lib.lib()
    buf, zeroed = np.zeros(64, np.int64), np.zeros(4096, np.uint8)  # both stay alive: the handle's mutex is in `zeroed`
    p, h = buf.ctypes.data, zeroed.ctypes.data

    def refused(rc, text):
        assert rc == INVALID
        assert text in L.clipgpu_last_error(), L.clipgpu_last_error()

    refused(L.clipgpu_index_enable_codes(None), b"NULL")
    refused(L.clipgpu_index_drop_codes(None), b"NULL")
    assert L.clipgpu_index_has_codes(None) == 0 and L.clipgpu_index_has_codes(h) == 0
    assert L.clipgpu_index_drop_codes(h) == 0  # nothing to free: no device call
    refused(L.clipgpu_index_get_codes(None, 0, 1, p, p), b"NULL")
    refused(L.clipgpu_index_get_codes(h, 0, 1, None, p), b"NULL")
    refused(L.clipgpu_index_get_codes(h, 0, 1, p, None), b"NULL")
    refused(L.clipgpu_index_get_codes(h, 0, 1, p, p), b"no codes")
    for fn, tail in ((L.clipgpu_index_search_coded, (None, None)), (L.clipgpu_index_search_coded_device, (p, p, None))):
        refused(fn(None, p, 1, 1, 1, 1.0, 0.0, None, p, p, *tail), b"NULL")
        refused(fn(h, None, 1, 1, 1, 1.0, 0.0, None, p, p, *tail), b"NULL")
        refused(fn(h, p, 1, 1, 1, 1.0, 0.0, None, None, p, *tail), b"NULL")
        refused(fn(h, p, 1, 1, 1, 1.0, 0.0, None, p, None, *tail), b"NULL")
        refused(fn(h, p, 0, 1, 1, 1.0, 0.0, None, p, p, *tail), b"Empty batch")
        for k in (0, 129, -2):
            refused(fn(h, p, 1, k, 128, 1.0, 0.0, None, p, p, *tail), b"k must be in 1..128")
        for k, refine in ((1, 0), (10, 9), (1, 129), (128, 200)):
            refused(fn(h, p, 1, k, refine, 1.0, 0.0, None, p, p, *tail), b"refine must be in k..128")
        refused(fn(h, p, 1, 10, 32, 1.0, 0.0, None, p, p, *tail), b"no codes")


def test_the_python_layer_checks_its_arguments_before_any_native_call(monkeypatch):
    from open_clip_inference import index as index_mod
    from open_clip_inference.error import ClipError

    class Stub(index_mod.EmbeddingIndex):
        def __init__(self, E=16):
            self._h = None
            self.E = E

        def __len__(self):
            return 40

    def no_lib():
        raise AssertionError("a native call was made")

    monkeypatch.setattr(index_mod, "lib", no_lib)
    ix, q = Stub(), np.zeros((2, 16), np.float32)
    with pytest.raises(ValueError, match="E <= 1024"):
        Stub(1040).enable_codes()
    for bad in (0, 129, -1):
        with pytest.raises(ValueError, match="k must be in 1..128"):
            ix.search_coded(q, bad)
        with pytest.raises(ValueError, match="k must be in 1..128"):
            ix.search_coded_device(1, 2, bad, 1, 1)
    for k, refine in ((10, 9), (1, 0), (5, 129)):
        with pytest.raises(ValueError, match="refine must be in k..128"):
            ix.search_coded(q, k, refine)
        with pytest.raises(ValueError, match="refine must be in k..128"):
            ix.search_coded_device(1, 2, k, 1, 1, refine)
    for bad in (2.0, "3", True):
        with pytest.raises(TypeError, match="refine must be an integer"):
            ix.search_coded(q, 5, bad)
        with pytest.raises(TypeError, match="k must be an integer"):
            ix.search_coded(q, bad)
    assert [index_mod.EmbeddingIndex._coded_args(k, None)[1] for k in (1, 8, 10, 32, 100, 128)] == [32, 32, 40, 128, 128, 128]
    with pytest.raises(TypeError, match="bool"):
        ix.search_coded(q, 5, allow=np.ones(40, np.uint8))
    with pytest.raises(ClipError, match="allow must have"):
        ix.search_coded(q, 5, allow=np.ones(39, bool))
    with pytest.raises(ClipError, match="Shape error"):
        ix.search_coded(np.zeros((2, 15), np.float32), 5)
    for call in (lambda: ix.enable_codes(), lambda: ix.search_coded(q, 5), lambda: ix.drop_codes(),
                 lambda: ix.has_codes, lambda: ix.codes(0, 3)):
        with pytest.raises(AssertionError, match="a native call was made"):  # good ones go on to the library
            call()


def test_clip_search_refuses_refine_with_nprobe():
    from open_clip_inference.clip import Clip
    with pytest.raises(ValueError, match="not both"):
        Clip.search(object(), object(), ["a"], 3, nprobe=2, refine=32)
