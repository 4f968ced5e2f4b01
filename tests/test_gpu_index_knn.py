"""Neighbours of stored rows and the k-NN graph (EmbeddingIndex.neighbors / knn_graph / neighbors_device,
Clip.similar / knn_graph; csrc/kernels/knn.hip) against a few lines of numpy over S = logits(rows, rows), the
pinned similarity kernel: per query id i the columns ok & (j != i) in stable descending order, cut to k, padded
with (-1, -inf).  Exact: indices by array_equal, scores on their uint32 views.  Shapes are the smallest that reach
the path named beside them."""
import functools

import numpy as np
import pytest

from tests.index_cases import (ROUND, assert_same, bits_equal_with_nans, padding, pattern, span_cols, special_rows,
                               tied_gallery, unit_rows)
from tests.index_range_cases import index_of, logits

pytestmark = pytest.mark.gpu
SCALE = 100.0


def oracle(S, ids, k, ok=None, valid=None):
    """ok: the candidate columns (live and allowed); valid: the query rows that get an answer at all."""
    ids = np.asarray(ids, np.int64)
    ok = np.ones(S.shape[1], bool) if ok is None else ok
    L = S[ids]
    order = np.argsort(-L, axis=1, kind="stable")
    keep = ok[order] & (order != ids[:, None])
    idx, score = padding(len(ids), k)
    for r in range(len(ids)):
        if valid is None or valid[r]:
            c = order[r][keep[r]][:k]
            idx[r, :len(c)], score[r, :len(c)] = c, L[r, c]
    return idx, score


@functools.lru_cache(maxsize=None)
def gallery300():
    g = unit_rows(np.random.default_rng(300), 300, 64)
    return g, logits(g, g, SCALE)


@pytest.mark.parametrize("N,E,k,cols", [
    (70, 16, 5, 0),        # one full panel and a ragged one, the self columns in both
    (200, 64, 16, 64),     # several spans, the merge runs; the self column in another span per panel
    (1000, 80, 128, 64),   # the cap of k, a ragged k slab, the largest lists, several launches
    (4097, 512, 10, 0),    # N one past a tile, 65 panels
    (40, 16, 64, 0),       # k above N - 1: padding after N - 1 real neighbours
])
def test_knn_graph_shapes(N, E, k, cols):
    g = unit_rows(np.random.default_rng(N + k), N, E)
    want = oracle(logits(g, g, SCALE), np.arange(N), k)
    span_cols(cols)
    try:
        with index_of(g) as ix:
            got = ix.knn_graph(k, SCALE)
    finally:
        span_cols(0)
    assert_same(got, want)
    assert (got[0] != np.arange(N)[:, None]).all()
    real = min(k, N - 1)
    assert (got[0][:, :real] >= 0).all() and (got[0][:, real:] == -1).all() and np.isneginf(got[1][:, real:]).all()


@pytest.mark.parametrize("ids", [[123], [299, 0, 64, 63, 7, 7, 128, 1, 250, 64, 5, 191, 192, 2, 299, 100, 31],
                                 list(range(299, 169, -2))], ids=["1", "17", "65"])
def test_neighbors_of_ids(ids):
    g, S = gallery300()
    with index_of(g) as ix:
        assert_same(ix.neighbors(ids, 10, SCALE), oracle(S, ids, 10))
        for bad in (-1, 300):
            with pytest.raises(Exception, match="id out of range"):
                ix.neighbors(ids + [bad], 10, SCALE)


@pytest.mark.parametrize("k", [10, 64])
def test_ties(k):
    """Eight distinct rows, 300 copies: every row has dozens of exact duplicates on both sides of its own id.  The
    stable order with exactly the self column missing; dropping the first hit of search(k + 1) does not give it."""
    _, g, _ = tied_gallery(np.random.default_rng(3), 300)
    want = oracle(logits(g, g, SCALE), np.arange(300), k)
    with index_of(g) as ix:
        assert_same(ix.knn_graph(k, SCALE), want)
        picks = [0, 150, 299, 150]
        assert_same(ix.neighbors(picks, k, SCALE), (want[0][picks], want[1][picks]))
        assert not np.array_equal(ix.search(g, k + 1, SCALE)[0][:, 1:], want[0])


def test_filter_and_removal():
    g, S = gallery300()
    allow = pattern(300)
    with index_of(g) as ix:
        first = ix.knn_graph(1, SCALE, allow=allow)[0][:, 0]
        gone = np.array([first[0], 9, 10, 299])  # row 0's best allowed neighbour, allowed rows, an unallowed one
        ix.remove(gone)
        live = np.ones(300, bool)
        live[gone] = False
        ok = allow & live
        got = ix.knn_graph(16, SCALE, allow=allow)
        assert_same(got, oracle(S, np.arange(300), 16, ok, valid=ok))
        assert got[0][0, 0] != first[0] and (got[0][~ok] == -1).all()
        ids = [1, 0, 9, 299, 2, 10]  # live but not allowed rows answer over the allowed columns; dead ones pad
        assert not allow[1] and not allow[2]
        assert_same(ix.neighbors(ids, 16, SCALE, allow=allow), oracle(S, ids, 16, ok, valid=live[ids]))
        assert_same(ix.neighbors(ids, 16, SCALE), oracle(S, ids, 16, live, valid=live[ids]))
        a, b = (int(i) for i in np.flatnonzero(live)[[70, 71]])
        one = np.zeros(300, bool)
        one[a] = True  # a single allowed row: its own result is all padding, every other row's is that row
        got = ix.neighbors([a, b], 3, SCALE, allow=one)
        assert_same(got, oracle(S, [a, b], 3, one))
        assert (got[0][0] == -1).all() and got[0][1, 0] == a


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_storage_types(dt):
    """A 16-bit index returns what an f32 index of the rounded rows returns, bit for bit; the special rows put NaN
    and inf rows among the queries and the columns."""
    g = unit_rows(np.random.default_rng(16), 300, 64)
    with index_of(g, dt) as ix:
        assert_same(ix.knn_graph(16, SCALE), oracle(logits(ROUND[dt](g), ROUND[dt](g), SCALE), np.arange(300), 16))
    s = ROUND[dt](special_rows())
    n = len(s)
    with index_of(special_rows(), dt) as ix, index_of(s) as ref:
        got, want = ix.knn_graph(n, SCALE), ref.knn_graph(n, SCALE)
        assert np.isnan(want[1]).any()
        assert_same(got, want)
        by_matrix = oracle(logits(s, s, SCALE), np.arange(n), n)
        assert np.array_equal(got[0], by_matrix[0])
        bits_equal_with_nans(got[1], by_matrix[1])


def test_exact_integers():
    """Rows of small integers: every dot is exact in f32 in any order, so int64 numpy holds the chain itself."""
    g = np.random.default_rng(64).integers(-3, 4, (200, 64)).astype(np.float32)
    S = (g.astype(np.int64) @ g.astype(np.int64).T).astype(np.float32)
    ids = [5, 199, 64, 5]
    with index_of(g) as ix:
        assert_same(ix.knn_graph(20), oracle(S, np.arange(200), 20))
        assert_same(ix.neighbors(ids, 20), oracle(S, ids, 20))


def test_device_form_with_an_id_out_of_range():
    import torch
    g, S = gallery300()
    ids = np.array([5, 300, 64, -1, 299, 1 << 40, 5], np.int64)
    inside = (ids >= 0) & (ids < 300)
    with index_of(g) as ix:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_ids = torch.from_numpy(ids).cuda()
            di = torch.full((len(ids), 10), -7, dtype=torch.int64, device="cuda")
            ds = torch.zeros((len(ids), 10), dtype=torch.float32, device="cuda")
            ix.neighbors_device(d_ids.data_ptr(), len(ids), 10, di.data_ptr(), ds.data_ptr(), SCALE, 0.0, s.cuda_stream)
            s.synchronize()
        got = di.cpu().numpy(), ds.cpu().numpy()
        assert_same(got, oracle(S, np.where(inside, ids, 0), 10, valid=inside))
        host = ix.neighbors(ids[inside], 10, SCALE)
        assert_same((got[0][inside], got[1][inside]), host)


def test_clip_similar_and_knn_graph():
    """The facade on the seeded tiny model, against the index calls on the same embeddings."""
    from open_clip_inference import Clip
    from tests.helpers import cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    with clip.build_index(images()) as index:
        n = len(index)
        idx, score = clip.knn_graph(index, 2)
        rows = index.rows()
        assert_same((idx, score), oracle(logits(rows, rows, 1.0), np.arange(n), 2))
        want = [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]
        assert clip.similar(index, list(range(n)), 2) == want and all(len(r) > 0 for r in want)
