"""The embedding index's probability search (EmbeddingIndex.search_probs; the PROBS kernels and the PROBS
merge of csrc/kernels/topk.hip) on the GPU.

Oracle (tests/index_probs_cases.py): the logits of the counted rows from similarity(..., "logits"), which is
pinned bit-equal to the search (for a 16-bit index on index.rows(), the rounded rows), then the
max-subtracted softmax and (M, S) in float64.  Required: |p - p*| <= B p* + 2^-126, |S - S*| <= B_S S*, M
bit-equal to the largest counted logit, with B derived there from the kernels' roundings (never from their
results) and capped at 2^-12.  At N <= 130 and scale 1 one column wrongly counted or dropped moves every
probability by at least e^-2 / N >= 1e-3, four times the cap.  Indices and logits must be those of
search(..., allow=) bit for bit; sigmoid probabilities those of similarity(..., "sigmoid") bit for bit."""
import functools

import numpy as np
import pytest

from tests import index_probs_cases as cases
from tests.index_cases import assert_same, pattern, route, routes_for, span_cols

pytestmark = pytest.mark.gpu

CUTS = (64, 0)  # clipgpu_test_topk_span_cols: 64-column spans, and the default cut


@functools.lru_cache(maxsize=None)
def data(N, dt="f32", E=64, Q=70, scale=1.0, order=None):
    """Gallery (as stored: rounded for a 16-bit index), queries, their logits and sigmoid matrices; computed
    once, shared, never written to.  order: +1 / -1 sorts the gallery by query 0's logit, ascending /
    descending."""
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    g, q = cases.rows(N, E, Q)
    if dt != "f32":
        with EmbeddingIndex(E, N, dtype=dt) as ix:
            ix.add(g)
            g = ix.rows()
    if order:
        g = g[np.argsort(order * similarity(q[:1], g, scale, 0.0, "logits", 1)[0], kind="stable")]
    g = np.ascontiguousarray(g)
    L = similarity(q, g, scale, 0.0, "logits", 1)
    P = similarity(q, g, scale, 0.0, "sigmoid", 1)
    for a in (g, L, P):
        a.setflags(write=False)
    return g, q, L, P


def check_search(ix, q, L, P, k, scale, allow, what):
    """One softmax and one sigmoid search against the oracle, search() and the sigmoid matrix."""
    live = np.ones(L.shape[1], bool) if allow is None else allow
    got = ix.search_probs(q, k, scale, 0.0, "softmax", allow=allow, return_norm=True)
    plain = ix.search(q, k, scale, 0.0, allow=allow)
    assert_same(got[:2], plain, what + " identity")
    B = cases.check(got, L[:len(q)], live & ix.is_live(), what)
    sg = ix.search_probs(q, k, scale, 0.0, "sigmoid", allow=allow, return_norm=True)
    assert_same(sg[:2], plain, what + " identity (sigmoid)")
    assert np.isnan(sg[3]).all(), what  # no normaliser: the array stays as it was handed in
    hit = sg[0] >= 0
    want = np.where(hit, np.take_along_axis(P[:len(q)], np.maximum(sg[0], 0), 1), np.float32(0))
    assert np.array_equal(sg[2].view(np.uint32), want.view(np.uint32)), what + " sigmoid"
    return got, B


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("N", [1, 50, 130])
def test_edges_at_scale_1(N, dt):
    """N = 130 leaves two columns in the last 64-tile and the last 16-tile; k >= N returns every row, and
    cases.check then also holds the sum of the probabilities to 1 within N B."""
    from open_clip_inference import EmbeddingIndex
    g, q, L, P = data(N, dt)
    assert np.abs(L).max() <= 1.0 + 1e-6
    try:
        for cols in CUTS:
            span_cols(cols)
            for nq in (1, 5, 16, 17, 70):
                for r in routes_for(nq):
                    with route(r), EmbeddingIndex(64, N, dtype=dt) as ix:
                        ix.add(g)
                        for k in (1, 10, 128):
                            _, B = check_search(ix, q[:nq], L, P, k, 1.0, None,
                                                f"N {N} {dt} nq {nq} k {k} route {r} span_cols {cols}")
                            assert B < 2.0 ** -16
    finally:
        span_cols(0)


def test_a_short_last_slab():
    from open_clip_inference import EmbeddingIndex
    g, q, L, P = data(130, "f32", 80, 17)
    for r, nq in ((1, 17), (1, 5), (2, 5)):
        with route(r), EmbeddingIndex(80, 130) as ix:
            ix.add(g)
            check_search(ix, q[:nq], L, P, 10, 1.0, None, f"E 80 route {r} nq {nq}")


@pytest.mark.parametrize("scale", [1.0, 100.0])
def test_257_queries_are_one_wide_chunk_and_one_few_query_chunk(scale):
    from open_clip_inference import EmbeddingIndex
    g, q, L, P = data(1037, "f32", 64, 257, scale)
    with EmbeddingIndex(64, 1037) as ix:
        ix.add(g)
        _, B = check_search(ix, q, L, P, 10, scale, None, f"257 queries scale {scale}")
    assert B <= cases.CAP


@pytest.mark.parametrize("order", [1, -1], ids=["ascending", "descending"])
def test_peaked_rows_at_scale_100(order):
    """The gallery sorted by query 0's logit: ascending, every tile raises that row's maximum (every lane
    rescales at every step); descending, none does."""
    from open_clip_inference import EmbeddingIndex
    g, q, L, P = data(1037, "f32", 64, 5, 100.0, order)
    assert (np.diff(L[0]) * order >= 0).all()
    try:
        for cols in CUTS:
            span_cols(cols)
            for r in (1, 2):
                with route(r), EmbeddingIndex(64, 1037) as ix:
                    ix.add(g)
                    got, B = check_search(ix, q, L, P, 10, 100.0, None, f"peaked {order} route {r} span_cols {cols}")
                    assert B <= cases.CAP and got[2][:, 0].min() > 0.01  # peaked: a few rows hold the mass
    finally:
        span_cols(0)


def sub_index_probs(q, g, keep, k, scale, dt="f32"):
    """search_probs of a fresh index that holds only the rows `keep` (ascending ids), indices mapped back."""
    from open_clip_inference import EmbeddingIndex
    A = np.flatnonzero(keep)
    with EmbeddingIndex(g.shape[1], len(A), dtype=dt) as ix:
        ix.add(g[A])
        idx, score, prob, norm = ix.search_probs(q, k, scale, 0.0, "softmax", return_norm=True)
    return np.where(idx >= 0, A[np.maximum(idx, 0)], -1).astype(np.int64), score, prob, norm


def filters(N):
    out = {"pattern": (pattern(N), None)}
    m = np.ones(N, bool)  # one whole 64-tile and (at 64-column spans) one whole span without an allowed row
    m[64:128] = False
    out["empty tile and span"] = (m, None)
    out["removed rows"] = (None, np.array([0, 5, 63, 64, 65, N // 2, N - 1]))
    m = pattern(N).copy()
    out["pattern and removed rows"] = (m, np.array([0, 3, 66, N - 1]))
    return out


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("N", [130, 300])
def test_filter_and_removal(N, scale):
    """The result is that of an index holding only the allowed live rows: indices and logits bit for bit,
    probabilities within 2 B (the two indices cut their spans differently)."""
    from open_clip_inference import EmbeddingIndex
    g, q, L, P = data(N, "f32", 64, 17, scale)
    try:
        for cols in (64, 0, 256):  # 256: the wide kernel skips an empty tile inside a span it works on
            span_cols(cols)
            for nq in (5, 17):
                for r in routes_for(nq):
                    for name, (allow, dead) in filters(N).items():
                        what = f"N {N} scale {scale} nq {nq} route {r} span_cols {cols} {name}"
                        with route(r), EmbeddingIndex(64, N) as ix:
                            ix.add(g)
                            if dead is not None:
                                ix.remove(dead)
                            got, B = check_search(ix, q[:nq], L, P, 10, scale, allow, what)
                            keep = (np.ones(N, bool) if allow is None else allow) & ix.is_live()
                            want = sub_index_probs(q[:nq], g, keep, 10, scale)
                        assert_same(got[:2], want[:2], what)
                        assert (np.abs(got[2].astype(np.float64) - want[2]) <= 2 * B * want[2] + cases.TINY).all(), what
                        assert np.array_equal(got[3][:, 0].view(np.uint32), want[3][:, 0].view(np.uint32)), what
    finally:
        span_cols(0)


@pytest.mark.parametrize("r", [1, 2], ids=["wide", "few-query"])
def test_nothing_allowed_is_empty_slots_and_no_error(r):
    from open_clip_inference import EmbeddingIndex
    g, q, L, P = data(130)
    with route(r), EmbeddingIndex(64, 130) as ix:
        ix.add(g)
        for allow in (np.zeros(130, bool), None):
            if allow is None:
                ix.remove(np.arange(130))
            for act in ("softmax", "sigmoid"):
                idx, score, prob, norm = ix.search_probs(q[:5], 10, 1.0, 0.0, act, allow=allow, return_norm=True)
                assert (idx == -1).all() and np.isneginf(score).all()
                assert np.array_equal(prob.view(np.uint32), np.zeros((5, 10), np.uint32))
                if act == "softmax":
                    assert np.isneginf(norm[:, 0]).all() and (norm[:, 1] == 0).all()


@pytest.mark.parametrize("r", [1, 2], ids=["wide", "few-query"])
def test_a_nan_row_makes_every_probability_nan(r):
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    g, q, _, _ = data(50)
    g = g.copy()
    g[20] = np.nan
    L = similarity(q[:5], g, 1.0, 0.0, "logits", 1)
    with route(r), EmbeddingIndex(64, 50) as ix:
        ix.add(g)
        got = ix.search_probs(q[:5], 50, 1.0, 0.0, "softmax", return_norm=True)
        assert_same(got[:2], ix.search(q[:5], 50, 1.0, 0.0))
        assert (got[0] >= 0).all() and np.isnan(got[2]).all() and np.isnan(got[3][:, 1]).all()
        cases.check(got, L, np.ones(50, bool), "NaN row")
        # without the row the probabilities are numbers again
        allow = np.ones(50, bool)
        allow[20] = False
        got = ix.search_probs(q[:5], 50, 1.0, 0.0, "softmax", allow=allow, return_norm=True)
        cases.check(got, L, allow, "NaN row filtered out")
        assert np.isfinite(got[2][:, :49]).all()


def test_infinite_logits():
    """-inf logits add nothing; a +inf logit makes every probability of its query NaN."""
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    g, q, _, _ = data(50)
    g, q = g.copy(), q[:5].copy()
    q[:, 0] = np.abs(q[:, 0]) + np.float32(0.1)
    for j in (3, 40):
        g[j] = 0
        g[j, 0] = -np.inf
    for r in (1, 2):
        with route(r), EmbeddingIndex(64, 50) as ix:
            ix.add(g)
            L = similarity(q, g, 1.0, 0.0, "logits", 1)
            assert np.isneginf(L[:, [3, 40]]).all()
            got = ix.search_probs(q, 50, 1.0, 0.0, "softmax", return_norm=True)
            cases.check(got, L, np.ones(50, bool), f"-inf rows route {r}")
            assert (got[2][:, -2:] == 0).all() and np.isfinite(got[2]).all()
            g2 = g.copy()
            g2[7] = 0
            g2[7, 0] = np.inf
            ix.set_rows([7], g2[7:8])
            L = similarity(q, g2, 1.0, 0.0, "logits", 1)
            got = ix.search_probs(q, 50, 1.0, 0.0, "softmax", return_norm=True)
            cases.check(got, L, np.ones(50, bool), f"+inf row route {r}")
            assert np.isnan(got[2]).all() and np.isposinf(got[3][:, 0]).all()


def test_device_form_after_an_add_on_another_stream():
    import torch
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.index import pack_allow
    g, q, L, P = data(300, "f32", 64, 17, 100.0)
    allow = pattern(300)
    with EmbeddingIndex(64, 300) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:].copy()).cuda()
            ix.add_device(rest.data_ptr(), 236, s1.cuda_stream)
        with torch.cuda.stream(s2):
            dq = torch.from_numpy(q[:17].copy()).cuda()
            da = torch.from_numpy(pack_allow(allow).view(np.int32)).cuda()
            di = torch.empty((17, 12), dtype=torch.int64, device="cuda")
            ds, dp = (torch.empty((17, 12), dtype=torch.float32, device="cuda") for _ in range(2))
            dn = torch.full((17, 2), 7.0, dtype=torch.float32, device="cuda")
            ix.search_probs_device(dq.data_ptr(), 17, 12, di.data_ptr(), ds.data_ptr(), dp.data_ptr(), 100.0, 0.0,
                                   "softmax", s2.cuda_stream, d_allow=da.data_ptr(), d_norm=dn.data_ptr())
            s2.synchronize()
            got = tuple(t.cpu().numpy() for t in (di, ds, dp, dn))
            cases.check(got, L[:17], allow, "search_probs_device")
            assert_same(got[:2], ix.search(q[:17], 12, 100.0, 0.0, allow=allow))
            dn.fill_(7.0)
            ix.search_probs_device(dq.data_ptr(), 17, 12, di.data_ptr(), ds.data_ptr(), dp.data_ptr(), 100.0, 0.0,
                                   "sigmoid", s2.cuda_stream, d_norm=dn.data_ptr())
            s2.synchronize()
            assert (dn.cpu().numpy() == 7.0).all()  # sigmoid leaves out_norm untouched
            idx = di.cpu().numpy()
            assert np.array_equal(dp.cpu().numpy().view(np.uint32), np.take_along_axis(P[:17], idx, 1).view(np.uint32))


def test_device_forms_run_past_the_first_chunk():
    """257 queries in the caller's device buffers: one 256-row chunk, then a one-row chunk that takes the
    few-query route and writes at the offsets q0 * k (indices, logits, probabilities) and q0 * 2 (norm).  All
    three device forms, on a non-default stream, under removed rows and an allow bitmap, equal the host forms
    bit for bit in every row (the host forms are held to the oracle at 257 queries above); the sigmoid search
    leaves d_norm as it was."""
    import torch
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.index import pack_allow
    N, Q, k, scale, sentinel = 300, 257, 12, 100.0, 7.0
    g, q = cases.rows(N, 64, Q)
    allow = pattern(N)
    with EmbeddingIndex(64, N) as ix:
        ix.add(g)
        ix.remove(np.array([0, 3, 66, 150, N - 1]))
        plain = ix.search(q, k, scale, 0.0, allow=allow)
        soft = ix.search_probs(q, k, scale, 0.0, "softmax", allow=allow, return_norm=True)
        sigm = ix.search_probs(q, k, scale, 0.0, "sigmoid", allow=allow)
        assert (plain[0][[0, 255, 256]] >= 0).all()  # rows of both chunks hold results
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dq = torch.from_numpy(q.copy()).cuda()
            da = torch.from_numpy(pack_allow(allow).view(np.int32)).cuda()
            di = torch.empty((Q, k), dtype=torch.int64, device="cuda")
            ds, dp = (torch.empty((Q, k), dtype=torch.float32, device="cuda") for _ in range(2))
            dn = torch.full((Q, 2), sentinel, dtype=torch.float32, device="cuda")

            def bits(*ts):
                s.synchronize()
                return [t.cpu().numpy() for t in ts]

            ix.search_device(dq.data_ptr(), Q, k, di.data_ptr(), ds.data_ptr(), scale, 0.0, s.cuda_stream,
                             d_allow=da.data_ptr())
            assert_same(bits(di, ds), plain, "search_device")
            di.fill_(-2)
            ds.fill_(sentinel)
            ix.search_probs_device(dq.data_ptr(), Q, k, di.data_ptr(), ds.data_ptr(), dp.data_ptr(), scale, 0.0,
                                   "softmax", s.cuda_stream, d_allow=da.data_ptr(), d_norm=dn.data_ptr())
            got = bits(di, ds, dp, dn)
            assert_same(got[:2], soft[:2], "search_probs_device softmax")
            assert np.array_equal(got[2].view(np.uint32), soft[2].view(np.uint32))
            assert np.array_equal(got[3].view(np.uint32), soft[3].view(np.uint32))
            di.fill_(-2)
            ds.fill_(sentinel)
            dp.fill_(sentinel)
            dn.fill_(sentinel)
            ix.search_probs_device(dq.data_ptr(), Q, k, di.data_ptr(), ds.data_ptr(), dp.data_ptr(), scale, 0.0,
                                   "sigmoid", s.cuda_stream, d_allow=da.data_ptr(), d_norm=dn.data_ptr())
            got = bits(di, ds, dp, dn)
            assert_same(got[:2], sigm[:2], "search_probs_device sigmoid")
            assert np.array_equal(got[2].view(np.uint32), sigm[2].view(np.uint32))
            assert (got[3] == sentinel).all()  # sigmoid leaves d_norm untouched


def test_clip_rank_and_classify_topk():
    """The facade on the seeded tiny model: the first k of rank_images_many / classify_many, probabilities
    within B plus the matrix path's own bound."""
    from open_clip_inference import Clip
    from open_clip_inference.engine import similarity
    from tests.helpers import make_model_dir
    from tests.helpers import TEXTS, cfg_with_tokenizer, images
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims, labels, k = images(), TEXTS[:4], 3
    scale, bias = clip._scale_bias()
    L = similarity(clip.vision.embed_images(ims), clip.text.embed_texts(labels), float(scale), float(bias), "logits", 1)
    R = float(L.max() - L.min())
    n = max(L.shape)
    tol = (cases.bound_for(n, R)[0] + cases.bound_matrix(n, R)) * cases.HI

    def close(got, want):
        assert [i for i, _ in got] == [i for i, _ in want]
        for (_, p), (_, p0) in zip(got, want):
            assert abs(p - p0) <= tol * max(p, p0) + cases.TINY, (p, p0, tol)

    with clip.build_index(ims) as index:
        ranked = clip.rank(index, labels[:2], k)
        allowed = clip.rank(index, labels[:2], k, allow=np.array([True, False, True, True]))
    many = clip.rank_images_many(ims, labels[:2])
    assert len(ranked) == 2
    for got, want in zip(ranked, many):
        assert len(got) == k
        close(got, want[:k])
    for got in allowed:  # three allowed rows: all of them, and their probabilities sum to one
        assert sorted(i for i, _ in got) == [0, 2, 3] and abs(sum(p for _, p in got) - 1.0) <= 1e-5
    with clip.build_label_index(labels) as label_index:
        assert len(label_index) == len(labels)
        top = clip.classify_topk(ims, label_index, k)
    many = clip.classify_many(ims, labels)
    assert len(top) == len(ims)
    for got, want in zip(top, many):
        assert len(got) == k
        close(got, [(labels.index(l), p) for l, p in want[:k]])
