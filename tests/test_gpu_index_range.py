"""The embedding index's range search and self-join on the GPU (EmbeddingIndex.range_search,
range_search_device, duplicates; csrc/kernels/range.hip), against the full logits matrix.

Oracle (tests/index_range_cases.py): L = similarity(q, g, scale, bias, "logits", 1), which is pinned bit-equal
to the search; for a 16-bit index on the rounded rows.  Per query the columns where live & allow & (L >= thr),
in stable descending order; for the join the pairs i < j of similarity(g, g) restricted the same way.  Every
comparison is exact: indices with array_equal, scores on uint32 views."""
import functools

import numpy as np
import pytest

from tests import index_range_cases as cases
from tests.index_cases import ROUND, pattern, route, routes_for, span_cols, tied_gallery, unit_rows

pytestmark = pytest.mark.gpu

NEG_INF, POS_INF = np.float32(-np.inf), np.float32(np.inf)


def up(x):
    return np.nextafter(np.float32(x), POS_INF)


@functools.lru_cache(maxsize=None)
def tied():
    """65 queries from a pool of four against eight distinct rows repeated 1000 times, their logits, and a
    threshold taken from the logits themselves; computed once, shared, never written to."""
    rng = np.random.default_rng(15)
    _, g, _ = tied_gallery(rng, 1000, 64)
    q = unit_rows(rng, 4, 64)[np.arange(65) % 4]
    L = cases.logits(q, g)
    thr = np.sort(np.unique(L[0]))[-4]  # the fourth largest of query 0's eight values
    assert (L == thr).sum() >= 100  # many scores exactly at the threshold, in every fourth query
    return g, q, L, thr


@pytest.mark.parametrize("Q", [1, 16, 17, 65])
def test_threshold_equality_and_ties(Q):
    g, q, L, thr = tied()
    at, above = cases.range_oracle(L[:Q], thr), cases.range_oracle(L[:Q], up(thr))
    ties = int((L[:Q] == thr).sum())
    assert ties > 0 and at[0][-1] - above[0][-1] == ties  # >= keeps them, the next f32 drops exactly them
    with cases.index_of(g) as ix:
        for r in routes_for(Q):
            with route(r):
                cases.assert_range(ix.range_search(q[:Q], thr, 100.0), at, f"route {r}")
                cases.assert_range(ix.range_search(q[:Q], up(thr), 100.0), above, f"route {r}, next f32")


@pytest.mark.parametrize("N", [1, 63, 65, 1000])
@pytest.mark.parametrize("E", [16, 80, 512])
def test_shapes(E, N):
    """E: one short slab; 64 + 16; several slabs.  N around the 64-column tile; 1000 rows in 16 spans of 64
    columns and in the default cut.  3 queries run either kernel, 70 are two query tiles of the wide one."""
    rng = np.random.default_rng(1000 * E + N)
    g, q = unit_rows(rng, N, E), unit_rows(rng, 70, E)
    L = cases.logits(q, g)
    thr = np.float32(np.quantile(L, 0.9))
    with cases.index_of(g) as ix:
        for Q in (3, 70):
            want = cases.range_oracle(L[:Q], thr)
            for cols in ((64, 0) if N == 1000 else (0,)):
                try:
                    span_cols(cols)
                    for r in routes_for(Q):
                        with route(r):
                            cases.assert_range(ix.range_search(q[:Q], thr, 100.0), want, f"Q {Q} cols {cols} route {r}")
                finally:
                    span_cols(0)


def test_chunking():
    """257 queries: one wide chunk of 256 and a one-row few-query chunk, on one counter."""
    rng = np.random.default_rng(257)
    g, q = unit_rows(rng, 300, 64), unit_rows(rng, 257, 64)
    L = cases.logits(q, g)
    thr = np.float32(np.quantile(L, 0.9))
    want = cases.range_oracle(L, thr)
    assert want[0][257] > want[0][256]  # the last query has results
    with cases.index_of(g) as ix:
        lims, idx, score = ix.range_search(q, thr, 100.0)
    assert lims[0] == 0 and (np.diff(lims) >= 0).all() and lims[-1] == len(idx) == len(score)
    assert lims[257] > lims[256]
    cases.assert_range((lims, idx, score), want)


def test_everything_and_nothing():
    rng = np.random.default_rng(4)
    g, q = unit_rows(rng, 1000, 64), unit_rows(rng, 3, 64)
    q[:, 0] = np.abs(q[:, 0]) + np.float32(0.01)  # a positive first component: +inf there scores +inf
    clean = cases.logits(q, g)
    assert np.isfinite(clean).all()
    g[700, 0] = np.nan
    g[333, 0] = np.inf
    L = cases.logits(q, g)
    assert np.isnan(L[:, 700]).all() and (L[:, 333] == POS_INF).all()
    want = cases.range_oracle(L, NEG_INF)
    assert want[0].tolist() == [0, 999, 1998, 2997]
    with cases.index_of(g) as ix:
        for r in (1, 2):
            with route(r):
                got = ix.range_search(q, NEG_INF, 100.0)
                cases.assert_range(got, want, f"route {r}")
                assert 700 not in got[1] and (got[1][got[0][:3]] == 333).all()  # no NaN row; +inf first
                # +inf as a threshold: only the +inf row
                cases.assert_range(ix.range_search(q, POS_INF, 100.0), cases.range_oracle(L, POS_INF))
        ix.set_rows([333, 700], unit_rows(rng, 2, 64))
        lims, idx, score = ix.range_search(q, POS_INF, 100.0)  # no inf scores any more: nothing
        assert lims.tolist() == [0, 0, 0, 0] and idx.size == 0 and score.size == 0


def test_filters_and_mutation():
    rng = np.random.default_rng(5)
    N = 1000
    g, q = unit_rows(rng, N, 64), unit_rows(rng, 20, 64)
    L = cases.logits(q, g)
    thr = np.float32(np.quantile(L, 0.9))
    dead = rng.choice(N, 150, replace=False)
    live = np.ones(N, bool)
    live[dead] = False
    allow = pattern(N)
    ok = live & allow
    with cases.index_of(g) as ix:
        ix.remove(dead)
        cases.assert_range(ix.range_search(q, thr, 100.0), cases.range_oracle(L, thr, live), "removed")
        got = ix.range_search(q, thr, 100.0, allow=allow)
        cases.assert_range(got, cases.range_oracle(L, thr, ok), "removed and filtered")
        # the result is that of an index holding only those rows, with positions mapped back
        with cases.index_of(g[ok]) as sub:
            lims, idx, score = sub.range_search(q, thr, 100.0)
        cases.assert_range(got, (lims, np.flatnonzero(ok)[idx], score), "sub-index")
        for r in (1, 2):  # both kernels' MASKED form
            with route(r):
                cases.assert_range(ix.range_search(q[:5], thr, 100.0, allow=allow), cases.range_oracle(L[:5], thr, ok))
        # set_rows revives a removed row: it appears again (an allowed one, set to the first query itself)
        back = int(dead[allow[dead]][0])
        assert back not in got[1]
        ix.set_rows([back], q[:1])
        g2, ok2 = g.copy(), ok.copy()
        g2[back], ok2[back] = q[0], True
        got = ix.range_search(q, thr, 100.0, allow=allow)
        cases.assert_range(got, cases.range_oracle(cases.logits(q, g2), thr, ok2), "revived")
        assert got[1][0] == back


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_16_bit_galleries(dt):
    rng = np.random.default_rng(6)
    g, q = unit_rows(rng, 1000, 80), unit_rows(rng, 20, 80)
    gr = ROUND[dt](g)
    L = cases.logits(q, gr)
    thr = np.float32(np.quantile(L, 0.9))
    want = cases.range_oracle(L, thr)
    with cases.index_of(gr) as ix32, cases.index_of(g, dt) as ix16:
        for Q in (5, 20):
            for r in routes_for(Q):
                with route(r):
                    a, b = ix32.range_search(q[:Q], thr, 100.0), ix16.range_search(q[:Q], thr, 100.0)
                    cases.assert_range(b, a, f"{dt} against f32 of the rounded rows, route {r}")
        cases.assert_range(b, want)


@functools.lru_cache(maxsize=None)
def dense():
    """About 3000 hits: 30 queries x 1000 rows at the 0.9 quantile."""
    rng = np.random.default_rng(7)
    g, q = unit_rows(rng, 1000, 64), unit_rows(rng, 30, 64)
    L = cases.logits(q, g)
    thr = np.float32(np.quantile(L, 0.9))
    return g, q, L, thr, cases.range_oracle(L, thr)


def test_capacity_of_the_host_form():
    from open_clip_inference.error import ResultOverflow
    g, q, L, thr, want = dense()
    total = int(want[0][-1])
    assert 2500 <= total <= 3500
    with cases.index_of(g) as ix:
        cases.assert_range(ix.range_search(q, thr, 100.0, max_results=total), want, "total == max_results")
        with pytest.raises(ResultOverflow, match=f"{total} results, max_results is {total - 1}") as e:
            ix.range_search(q, thr, 100.0, max_results=total - 1)
        assert e.value.needed == total
        with pytest.raises(ResultOverflow) as e:  # far too small: the count is still exact
            ix.range_search(q, thr, 100.0, max_results=1)
        assert e.value.needed == total
        cases.assert_range(ix.range_search(q, thr, 100.0, max_results=total), want, "after the overflows")


def test_capacity_guard_and_stream_order_of_the_device_form():
    """capacity = 10 records followed by a 64-record guard, about 3000 true hits: the total is exact, exactly
    10 records are written, each one of the oracle's, and the guard is untouched.  The rows arrive by
    add_device on one stream and the search runs on another."""
    import torch
    from open_clip_inference import EmbeddingIndex
    g, q, L, thr, want = dense()
    total = int(want[0][-1])
    lims, idx, score = want
    truth = {(qi, int(j)): int(s) for qi in range(len(q))
             for j, s in zip(idx[lims[qi]:lims[qi + 1]], score[lims[qi]:lims[qi + 1]].view(np.uint32))}
    cap, guard = 10, 64
    SQ, SR, SS = -7, -9, np.float32(-12345.0)
    with EmbeddingIndex(64, 1000) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:]).cuda()
            ix.add_device(rest.data_ptr(), 936, s1.cuda_stream)
        with torch.cuda.stream(s2):
            dq = torch.from_numpy(q).cuda()
            oq = torch.full((cap + guard,), SQ, dtype=torch.int32, device="cuda")
            orow = torch.full((cap + guard,), SR, dtype=torch.int32, device="cuda")
            os_ = torch.full((cap + guard,), float(SS), dtype=torch.float32, device="cuda")
            tot = torch.full((1,), 123456789, dtype=torch.int64, device="cuda")  # the call zeroes it
            ix.range_search_device(dq.data_ptr(), len(q), thr, cap, oq.data_ptr(), orow.data_ptr(), os_.data_ptr(),
                                   tot.data_ptr(), 100.0, 0.0, s2.cuda_stream)
            s2.synchronize()
        assert len(ix) == 1000
        hq, hr, hs = oq.cpu().numpy(), orow.cpu().numpy(), os_.cpu().numpy()
        assert int(tot.cpu().numpy()[0]) == total
        assert (hq[cap:] == SQ).all() and (hr[cap:] == SR).all() and (hs[cap:] == SS).all()  # the guard
        recs = list(zip(hq[:cap].tolist(), hr[:cap].tolist(), hs[:cap].view(np.uint32).tolist()))
        assert len(set(r[:2] for r in recs)) == cap  # ten written, all different
        for qi, j, bits in recs:
            assert truth.get((qi, j)) == bits, (qi, j)
        # a capacity that holds everything: the complete set, in some order
        with torch.cuda.stream(s2):
            big = total + 5
            oq = torch.full((big,), SQ, dtype=torch.int32, device="cuda")
            orow = torch.full((big,), SR, dtype=torch.int32, device="cuda")
            os_ = torch.full((big,), float(SS), dtype=torch.float32, device="cuda")
            ix.range_search_device(dq.data_ptr(), len(q), thr, big, oq.data_ptr(), orow.data_ptr(), os_.data_ptr(),
                                   tot.data_ptr(), 100.0, 0.0, s2.cuda_stream)
            s2.synchronize()
        hq, hr, hs = oq.cpu().numpy(), orow.cpu().numpy(), os_.cpu().numpy()
        assert int(tot.cpu().numpy()[0]) == total and (hq[total:] == SQ).all()
        got = dict(((a, b), c) for a, b, c in zip(hq[:total].tolist(), hr[:total].tolist(),
                                                  hs[:total].view(np.uint32).tolist()))
        assert got == truth


def copies(g, thr=np.float32(0.99)):
    """The self-join oracle of a gallery (as stored) at scale 1, bias 0."""
    S = cases.logits(g, g, 1.0, 0.0)
    return S, cases.join_oracle(S, thr)


@pytest.mark.parametrize("N", [257, 266, 513])
def test_self_join_returns_every_pair_of_copies(N):
    """The chunk boundary at 256 rows falls inside (257: a one-row last chunk; 266: a ten-row one, on the
    few-query kernel) and at the edge (513).  At a threshold just below 1 every pair of copies of a base row
    is returned, and no (i, i)."""
    rng = np.random.default_rng(N)
    base, g, d = tied_gallery(rng, N, 64)
    assert (d - np.eye(8)).max() < 0.9  # distinct base rows are far below the threshold
    S, want = copies(g)
    which = np.array([int(np.argmax((base == row).all(axis=1))) for row in g])
    n = np.bincount(which, minlength=8)
    assert len(want[0]) == int((n * (n - 1) // 2).sum()) and (want[0][:, 0] < want[0][:, 1]).all()
    with cases.index_of(g) as ix:
        cases.assert_pairs(ix.duplicates(0.99), want)
        for r in (1, 2):
            with route(r):
                cases.assert_pairs(ix.duplicates(0.99), want, f"route {r}")
        # with removed rows and a filter
        dead = rng.choice(N, 40, replace=False)
        ok = pattern(N)
        ok[dead] = False
        ix.remove(dead)
        cases.assert_pairs(ix.duplicates(0.99, allow=pattern(N)), cases.join_oracle(S, np.float32(0.99), ok), "filtered")
    with cases.index_of(g, "f16") as ix:
        gr = ix.rows()
        assert np.array_equal(gr.view(np.uint32), ROUND["f16"](g).view(np.uint32))
        # the rounded copies are still copies, but their self-dot is no longer 1 to the last bit: a lower cut
        cases.assert_pairs(ix.duplicates(0.98), copies(gr, np.float32(0.98))[1], "f16")


def test_self_join_of_one_row_and_off_the_ties():
    from open_clip_inference.error import ResultOverflow
    rng = np.random.default_rng(8)
    g = unit_rows(rng, 300, 64)
    with cases.index_of(g[:1]) as ix:
        pairs, score = ix.duplicates(NEG_INF)
        assert pairs.shape == (0, 2) and pairs.dtype == np.int64 and score.size == 0
    S = cases.logits(g, g, 1.0, 0.0)
    assert np.array_equal(S.view(np.uint32), S.T.view(np.uint32))  # symmetric bit for bit
    off = np.sort(S[np.triu_indices(300, 1)])
    thr = off[-50]  # a threshold that is one of the scores: >= keeps it, the next f32 drops it
    at, above = cases.join_oracle(S, thr), cases.join_oracle(S, up(thr))
    assert len(at[0]) >= 50 and len(above[0]) < len(at[0])
    with cases.index_of(g) as ix:
        cases.assert_pairs(ix.duplicates(thr), at)
        cases.assert_pairs(ix.duplicates(up(thr)), above)
        cases.assert_pairs(ix.duplicates(thr, 100.0, -3.0), cases.join_oracle(cases.logits(g, g, 100.0, -3.0), thr))
        # everything: 300 * 299 / 2 pairs; one fewer than that is refused with the exact count
        cases.assert_pairs(ix.duplicates(NEG_INF, max_pairs=44850), cases.join_oracle(S, NEG_INF))
        with pytest.raises(ResultOverflow, match="44850 results, max_pairs is 44849") as e:
            ix.duplicates(NEG_INF, max_pairs=44849)
        assert e.value.needed == 44850


def test_clip_search_above_and_find_duplicates():
    """The facade on the seeded tiny model, against range_search and duplicates of the same embeddings."""
    from open_clip_inference import Clip
    from tests.helpers import TEXTS, cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims, texts = images(), TEXTS[:3]
    ims = list(ims) + [ims[0]]  # a duplicate picture
    scale, bias = clip._scale_bias()
    te = clip.text.embed_texts(texts)
    with clip.build_index(ims) as index:
        n = len(index)
        L = cases.logits(te, index.rows(), float(scale), float(bias))
        thr = float(np.median(L))
        lims, idx, score = index.range_search(te, thr, float(scale), float(bias))
        cases.assert_range((lims, idx, score), cases.range_oracle(L, thr))
        got = clip.search_above(index, texts, thr)
        assert got == [[(int(i), float(s)) for i, s in zip(idx[a:b], score[a:b])] for a, b in zip(lims[:-1], lims[1:])]
        assert sum(len(r) for r in got) == lims[-1] > 0
        allow = np.arange(n) != int(idx[0])
        assert all(i != int(idx[0]) for r in clip.search_above(index, texts, thr, allow=allow) for i, _ in r)
        pairs, cos = index.duplicates(0.999)
        found = clip.find_duplicates(index, 0.999)
        assert found == [(int(i), int(j), float(c)) for (i, j), c in zip(pairs, cos)]
        assert (0, n - 1) in [(i, j) for i, j, _ in found]
        cases.assert_pairs((pairs, cos), cases.join_oracle(cases.logits(index.rows(), index.rows(), 1.0, 0.0), 0.999))
