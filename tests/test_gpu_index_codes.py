"""The embedding index's int8 codes and coded search on the GPU (EmbeddingIndex.enable_codes, codes, search_coded,
search_coded_device, Clip.search(refine=); csrc/kernels/codes.hip and the re-rank through csrc/kernels/probe.hip),
against the oracles of tests/index_codes_cases.py.

The codes, the candidates and the coarse scores are integers and single f32 operations, restated in numpy; the
logits of the re-rank come from similarity(queries, rows as stored), the library's pinned function.  Every
comparison is exact: codes and ids with array_equal, scores on their uint32 views (index_cases.assert_same).
tests/test_cpu_index_codes.py shows that each assertion here catches the matching mutant of its oracle."""
from contextlib import contextmanager

import numpy as np
import pytest

from tests import index_codes_cases as cases
from tests.index_cases import ROUND, assert_same, logits_oracle, padding, pattern, route, span_cols, tied_gallery

pytestmark = pytest.mark.gpu

E0, N0, Q0, K0, R0 = 16, 300, 5, 10, 32  # the defaults of the sweeps: one axis moves, the others stay


@contextmanager
def spans(cols):
    span_cols(cols)
    try:
        yield
    finally:
        span_cols(0)


@contextmanager
def parts(n):
    cases.hook("clipgpu_test_probe_parts", n)
    try:
        yield
    finally:
        cases.hook("clipgpu_test_probe_parts", 0)


def coded_index(g, dt="f32", capacity=None):
    ix = cases.index_of(g, dt, capacity)
    ix.enable_codes()
    return ix


def expect(ix, stored, q, k, refine, scale=100.0, bias=0.0, allow=None):
    """The contract restated: the plain search's oracle over each query's candidates, the candidates from the
    oracle codes of the rows as stored, over the rows that are live now and allowed."""
    ok = ix.is_live() if allow is None else ix.is_live() & allow
    return cases.expect(cases.logits(q, stored, scale, bias), stored, q, ok, k, refine, neg=scale < 0)


def check(ix, stored, q, k, refine, scale=100.0, bias=0.0, allow=None, what=""):
    want, cand, cs = expect(ix, stored, q, k, refine, scale, bias, allow)
    idx, score, gc, gs = ix.search_coded(q, k, refine, scale, bias, allow=allow, return_candidates=True)
    assert gc.dtype == np.int64 and gs.dtype == np.float32
    assert np.array_equal(gc, cand), what
    assert np.array_equal(gs.view(np.uint32), cs.view(np.uint32)), what
    assert_same((idx, score), want, what)
    assert_same(ix.search_coded(q, k, refine, scale, bias, allow=allow), want, what)
    return want, cand


def check_codes(ix, stored, what=""):
    want = cases.codes_oracle(stored)
    got = ix.codes()
    assert got[0].dtype == np.int8 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


# ---- the codes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("E", [16, 80, 512])
def test_codes_are_the_oracles(E, dt):
    """Padding to 64; 64 + 16; eight steps.  The specials first, then rows with different maxima."""
    rows = np.concatenate([cases.special_rows(E), cases.gallery(E, N0 - 12)])
    stored = rows if dt == "f32" else ROUND[dt](rows)
    with coded_index(rows, dt) as ix:
        assert ix.has_codes
        check_codes(ix, stored)
        part = ix.codes(7, 40)
        want = cases.codes_oracle(stored[7:47])
        assert np.array_equal(part[0], want[0]) and np.array_equal(part[1], want[1])
        if dt != "f32":
            with coded_index(stored) as ix32:
                for a, b in zip(ix.codes(), ix32.codes()):
                    assert np.array_equal(a, b)


def test_wide_rows_and_the_width_limit():
    """E = 1024: sixteen steps, the widest instantiation; and every code at its extreme, the largest |d|."""
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    g, q = cases.gallery(1024, 40).copy(), cases.queries(1024, 3).copy()
    g[5], q[1] = 1.0, -1.0  # codes all 127 and all -127: d = -1024 * 127^2
    with coded_index(g) as ix:
        check_codes(ix, g)
        for scale in (100.0, -100.0):
            check(ix, g, q, 5, 8, scale)
    with EmbeddingIndex(1040, 4) as ix:
        with pytest.raises(ValueError, match="E <= 1024"):
            ix.enable_codes()
        from open_clip_inference import _lib
        assert _lib.lib().clipgpu_index_enable_codes(ix.handle) == 1 and not ix.has_codes
        with pytest.raises(ClipError, match="at most 1024"):
            _lib.check(_lib.lib().clipgpu_index_enable_codes(ix.handle))


# ---- candidates, coarse scores and results: one sweep per axis ------------------------------------------
@pytest.mark.parametrize("N", [1, 17, 129, 300, 1200])
def test_gallery_sizes(N):
    g, q = cases.gallery(E0, N), cases.queries(E0, Q0)
    with coded_index(g) as ix:
        check(ix, g, q, min(K0, R0), R0)
        check(ix, g, q, 1, 1)
        if N <= R0:  # at most refine rows: the plain search
            assert_same(ix.search_coded(q, K0, R0, 100.0, 0.0), ix.search(q, K0, 100.0, 0.0))


@pytest.mark.parametrize("Q", [1, 5, 16, 17, 65, 260])
def test_query_counts(Q):
    """Around the 16-row route, past one four-wave block, past one chunk of 256 rows."""
    g, q = cases.gallery(E0, N0), cases.queries(E0, Q)
    with coded_index(g) as ix:
        check(ix, g, q, K0, R0)


@pytest.mark.parametrize("k,refine", [(1, 1), (1, 16), (10, 16), (16, 17), (17, 17), (10, 128), (17, 128), (128, 128)])
def test_result_and_candidate_counts(k, refine):
    """Each list capacity of the scan and of the re-rank."""
    g = cases.gallery(E0, N0)
    with coded_index(g) as ix:
        for Q in (Q0, 17):
            check(ix, g, cases.queries(E0, Q), k, refine)


@pytest.mark.parametrize("E", [80, 512])
def test_embedding_widths(E):
    g, q = cases.gallery(E, N0), cases.queries(E, 17)
    with coded_index(g) as ix:
        check(ix, g, q, K0, R0)
        check(ix, g, q[:Q0], K0, R0, allow=pattern(N0))


@pytest.mark.parametrize("scale", [100.0, -100.0, 0.0])
def test_the_sign_of_the_logit_scale(scale):
    """A negative scale turns the coarse order round; 0 counts as positive (and every logit is the bias)."""
    g = cases.gallery(E0, N0)
    with coded_index(g) as ix:
        for Q in (Q0, 17):
            check(ix, g, cases.queries(E0, Q), K0, R0, scale, 0.5)


def test_equal_coarse_scores_come_out_by_row_id_across_span_seams():
    rng = np.random.default_rng(3)
    base, g, _ = tied_gallery(rng, N0, 64)
    q = np.concatenate([base[:3], cases.queries(64, 14)])
    with coded_index(g) as ix:
        for Q in (3, 17):
            for cols in (0, 64, 128):
                with spans(cols):
                    want, cand = check(ix, g, q[:Q], K0, R0, what=f"Q {Q} span {cols}")
                    assert (np.diff(cand[:3, :20], axis=1) > 0).all() and cand[:3, :20].max() > 128


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_a_16_bit_index_searches_as_the_f32_index_of_its_rounded_rows(dt):
    g, q = cases.gallery(80, N0), cases.queries(80, Q0)
    r = ROUND[dt](g)
    with coded_index(g, dt) as ix16, coded_index(r) as ix32:
        got = ix16.search_coded(q, K0, R0, 100.0, 0.0, return_candidates=True)
        want = ix32.search_coded(q, K0, R0, 100.0, 0.0, return_candidates=True)
        assert_same(got[:2], want[:2])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        check(ix16, r, q, K0, R0)


# ---- the contract against the existing search -----------------------------------------------------------
def test_each_query_equals_a_filtered_search_of_its_candidates():
    g, q = cases.gallery(E0, N0), cases.queries(E0, Q0)
    with coded_index(g) as ix:
        ix.remove([3, 4, 200])
        idx, score, cand, _ = ix.search_coded(q, K0, R0, 100.0, -3.0, return_candidates=True)
        for i in range(3):
            mask = np.isin(np.arange(N0), cand[i])
            assert_same((idx[i:i + 1], score[i:i + 1]), ix.search(q[i:i + 1], K0, 100.0, -3.0, allow=mask), f"query {i}")


@pytest.mark.parametrize("E", [16, 80, 512])
def test_a_planted_gap_above_the_error_bound_gives_the_plain_search(E):
    """Derived, not measured: index_codes_cases.planted_gap asserts gap > 2 B, so refine = k loses nothing."""
    rows, q, gap, B = cases.planted_gap(E, N0, Q0, K0)
    with coded_index(rows) as ix:
        assert_same(ix.search_coded(q, K0, K0, 100.0, 0.0), ix.search(q, K0, 100.0, 0.0))
        assert_same(ix.search_coded(q, K0, K0, 1.0, 0.0), ix.search(q, K0, 1.0, 0.0))


# ---- the seams of the launches --------------------------------------------------------------------------
def test_the_result_does_not_depend_on_spans_routes_or_parts():
    g = cases.gallery(E0, 1200)
    allow = pattern(1200)
    with coded_index(g) as ix:
        for Q in (Q0, 17):
            q = cases.queries(E0, Q)
            want = expect(ix, g, q, K0, 128)
            masked = expect(ix, g, q, K0, 128, allow=allow)
            for cols in (64, 128, 1 << 20):  # 19 spans, 10 spans, one span
                for r in ((1, 2) if Q <= 16 else (0,)):
                    with spans(cols), route(r):
                        what = f"Q {Q} span {cols} route {r}"
                        got = ix.search_coded(q, K0, 128, 100.0, 0.0, return_candidates=True)
                        assert_same(got[:2], want[0], what)
                        assert np.array_equal(got[2], want[1]) and np.array_equal(got[3], want[2]), what
                        got = ix.search_coded(q, K0, 128, 100.0, 0.0, allow=allow, return_candidates=True)
                        assert_same(got[:2], masked[0], what)
                        assert np.array_equal(got[2], masked[1]) and np.array_equal(got[3], masked[2]), what
            for n in (1, 3, 100):  # 100 parts: most blocks of the re-rank are empty
                with parts(n):
                    assert_same(ix.search_coded(q, K0, 128, 100.0, 0.0), want[0], f"parts {n}")
                    assert_same(ix.search_coded(q, K0, 128, 100.0, 0.0, allow=allow), masked[0], f"masked, parts {n}")


# ---- filters and removal --------------------------------------------------------------------------------
def test_filters_and_removal():
    g, q = cases.gallery(E0, N0), cases.queries(E0, Q0)
    allow = pattern(N0)
    with coded_index(g) as ix:
        check(ix, g, q, K0, R0, allow=allow)
        first = ix.search_coded(q, 1, R0, 100.0, 0.0)[0][:, 0]
        assert (first >= 0).all()
        ix.remove(first)  # every query's best row
        for kw in ({}, {"allow": allow}):
            want, cand = check(ix, g, q, K0, R0, **kw)
            assert not np.isin(want[0], first).any() and not np.isin(cand, first).any()
        # every row filtered: padding, no error
        got = ix.search_coded(q, K0, R0, 100.0, 0.0, allow=np.zeros(N0, bool), return_candidates=True)
        assert_same(got[:2], padding(Q0, K0))
        assert (got[2] == -1).all() and np.isneginf(got[3]).all()
        # fewer allowed rows than k: padding behind them
        few = np.zeros(N0, bool)
        few[[1, 50, 299]] = True
        want, cand = check(ix, g, q, K0, R0, allow=few)
        assert (want[0][:, 3:] == -1).all() and (want[0][:, :3] >= 0).all() and (cand[:, 3:] == -1).all()
        ix.remove(np.arange(N0))
        assert_same(ix.search_coded(q, K0, R0, 100.0, 0.0), padding(Q0, K0))


# ---- maintenance ----------------------------------------------------------------------------------------
def test_the_codes_follow_add_set_rows_and_clear():
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    g, q = cases.gallery(E0, N0), cases.queries(E0, Q0)
    other = cases.gallery(E0, 40, seed=1)
    with EmbeddingIndex(E0, N0) as ix:
        assert not ix.has_codes
        with pytest.raises(ClipError, match="no codes"):
            ix.search_coded(q, K0, R0)
        ix.enable_codes()  # on an empty index
        assert ix.has_codes
        with pytest.raises(ClipError, match="Empty batch"):
            ix.search_coded(q, K0, R0)
        ix.add(g[:100])
        check_codes(ix, ix.rows(), "first piece")
        check(ix, g[:100], q, K0, R0)
        ix.add(g[100:])
        stored = g.copy()
        check_codes(ix, stored, "second piece")
        check(ix, stored, q, K0, R0)
        ix.enable_codes()  # twice: a no-op
        check_codes(ix, stored)
        best = ix.search_coded(q, 1, R0, 100.0, 0.0)[0][:, 0]
        live_ids = np.unique(best)
        ix.set_rows(live_ids, -g[live_ids])  # live slots: every query's best row becomes its worst
        stored[live_ids] = -g[live_ids]
        assert np.array_equal(ix.rows(), stored)
        check_codes(ix, ix.rows(), "set_rows on live slots")
        want, cand = check(ix, stored, q, K0, R0)
        assert all(best[i] not in cand[i] for i in range(Q0))  # no query keeps the row that was its best
        check(ix, stored, q, K0, K0)  # refine = k: a stale candidate would cost a result
        ix.remove([7, 8, 150])
        check(ix, stored, q, K0, R0)
        ix.set_rows([8, 150], other[:2])  # removed slots: live again, with new codes
        stored[[8, 150]] = other[:2]
        check_codes(ix, ix.rows(), "set_rows on removed slots")
        assert ix.live == N0 - 1
        check(ix, stored, q, K0, R0)
        ix.clear()
        assert ix.has_codes and len(ix) == 0
        ix.add(other)
        check_codes(ix, other, "after clear")
        check(ix, other, q, K0, R0)
        ix.drop_codes()
        assert not ix.has_codes
        with pytest.raises(ClipError, match="no codes"):
            ix.search_coded(q, K0, R0)
        with pytest.raises(ClipError, match="no codes"):
            ix.codes()
        assert_same(ix.search(q, K0, 100.0, 0.0), logits_oracle(cases.logits(q, other, 100.0), np.ones(40, bool), K0))
        ix.enable_codes()  # again, on a filled index
        check_codes(ix, other)
        check(ix, other, q, K0, R0)


def test_add_device_codes_the_rows_it_writes():
    import torch
    g, q = cases.gallery(E0, N0), cases.queries(E0, Q0)
    with coded_index(g[:200], capacity=N0) as ix:
        d = torch.from_numpy(g[200:].copy()).cuda()
        ix.add_device(d.data_ptr(), 100, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        check_codes(ix, g)
        check(ix, g, q, K0, R0)


# ---- the device form ------------------------------------------------------------------------------------
def test_the_device_form_writes_only_its_outputs_and_takes_a_device_filter():
    import torch
    from open_clip_inference.index import pack_allow
    g, q = cases.gallery(E0, N0), cases.queries(E0, 17)
    allow = pattern(N0)
    guard, fill = 8, 0xA5
    with coded_index(g) as ix:
        ix.remove([0, 9, 150])
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dq = torch.from_numpy(q.copy()).cuda()
            da = torch.from_numpy(pack_allow(allow).view(np.int32)).cuda()

            def filled(cols, dtype):
                size = torch.empty((), dtype=dtype).element_size()
                return torch.full((17 + guard, cols * size), fill, dtype=torch.uint8, device="cuda").view(dtype)

            oi, os_ = filled(K0, torch.int64), filled(K0, torch.float32)
            oc, of = filled(R0, torch.int64), filled(R0, torch.float32)
            ix.search_coded_device(dq.data_ptr(), 17, K0, oi.data_ptr(), os_.data_ptr(), R0, 100.0, 0.0, s.cuda_stream,
                                   da.data_ptr(), oc.data_ptr(), of.data_ptr())
            oi2, os2 = filled(K0, torch.int64), filled(K0, torch.float32)
            ix.search_coded_device(dq.data_ptr(), 17, K0, oi2.data_ptr(), os2.data_ptr(), R0, 100.0, 0.0, s.cuda_stream,
                                   da.data_ptr())  # NULL out_cand / out_coarse
        s.synchronize()
        want, cand, cs = expect(ix, g, q, K0, R0, allow=allow)
        hi, hs, hc, hf = (t.cpu().numpy() for t in (oi, os_, oc, of))
        assert_same((hi[:17], hs[:17]), want)
        assert np.array_equal(hc[:17], cand) and np.array_equal(hf[:17].view(np.uint32), cs.view(np.uint32))
        for a in (hi, hs, hc, hf, oi2.cpu().numpy(), os2.cpu().numpy()):
            assert (a[17:].view(np.uint8) == fill).all()  # nothing past [nq][k] / [nq][refine] is written
        assert_same((oi2.cpu().numpy()[:17], os2.cpu().numpy()[:17]), want)
        assert_same(ix.search_coded(q, K0, R0, 100.0, 0.0, allow=allow), want)


def test_clip_search_with_refine():
    """The facade on the seeded tiny model: refine=None is today's path; refine >= the rows gives the same result."""
    from open_clip_inference import Clip
    from tests.helpers import cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims = list(images())
    texts = ["a photo of a cat", "a dog"]
    with clip.build_index(ims) as index:
        index.enable_codes()
        plain = clip.search(index, texts, 3)
        assert plain == clip.search(index, texts, 3, refine=None) and clip.search(index, texts, 3, refine=32) == plain
        scale, bias = clip._scale_bias()
        idx, score = index.search_coded(clip.text.embed_texts(texts), 1, 1, float(scale), float(bias))
        want = [[(int(i), float(v)) for i, v in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]
        assert clip.search(index, texts, 1, refine=1) == want and all(want)
        with pytest.raises(ValueError, match="not both"):
            clip.search(index, texts, 3, nprobe=1, refine=32)
