"""The few-query phase-1 kernel of the embedding index (topk_narrow_kernel, csrc/kernels/topk.hip)
against the wide kernel and against the sorted logits matrix.  clipgpu_test_topk_route runs either
kernel on one input (1 = wide, 2 = few-query wherever at most 16 rows are launched); the route must
be invisible: every comparison is == on indices and on uint32 views of scores."""
import numpy as np
import pytest

from tests.index_cases import ROUND, assert_same, expected, route, search16, search_once, span_cols, tied_gallery, \
    unit_rows

pytestmark = pytest.mark.gpu


def narrow_rows():
    """kNarrowRows: launches of at most this many rows take the few-query kernel by default."""
    from open_clip_inference import _lib
    n = _lib.lib().clipgpu_test_topk_narrow_rows()
    assert 1 <= n <= 16
    return n


# every value of every axis at least once, the extremes combined, N < k twice; k covers both sides of
# every list capacity (16 / 32 / 64 / 128)
CASES = [(1, 1, 16, 1), (16, 5000, 512, 128), (15, 65, 48, 33), (2, 63, 144, 64), (1, 64, 48, 17),
         (16, 1000, 16, 32), (2, 1000, 512, 16), (15, 5000, 144, 65), (1, 63, 16, 128), (16, 64, 512, 1)]


def test_the_cases_cover_the_axes():
    for axis, vals in enumerate(([1, 2, 15, 16], [1, 63, 64, 65, 1000, 5000], [16, 48, 144, 512],
                                 [1, 16, 17, 32, 33, 64, 65, 128])):
        assert {c[axis] for c in CASES} == set(vals)
    assert any(c[1] < c[3] for c in CASES)


@pytest.mark.parametrize("Q,N,E,k", CASES)
def test_both_routes_give_the_sorted_logits(Q, N, E, k):
    rng = np.random.default_rng(100 * Q + N + k)
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    want = expected(q, g, k, 100.0, 0.0)
    got = {}
    for r in (1, 2):
        with route(r):
            got[r] = search_once(q, g, k)
        assert_same(got[r], want, f"route {r}")
    assert_same(got[1], got[2], "wide vs few-query")
    if N < k:
        assert (got[2][0][:, N:] == -1).all() and np.isneginf(got[2][1][:, N:]).all()


def test_chunk_seam():
    """Default dispatch around the route threshold and around the 256-row chunking: 257 queries are
    one wide chunk and a one-row chunk; 272 / 273 end in a 16- / 17-row chunk."""
    n = narrow_rows()
    rng = np.random.default_rng(9)
    g = unit_rows(rng, 700, 64)
    q = unit_rows(rng, 256 + 17, 64)
    want = expected(q, g, 10, 100.0, 0.0)
    for Q in (n, n + 1, 256 + 1, 256 + 16, 256 + 17):
        assert_same(search_once(q[:Q], g, 10), (want[0][:Q], want[1][:Q]), f"Q {Q}")


def line_gallery(rng, N, E, increasing):
    """Rows c_j * u for a unit u with c_j strictly monotone in j: with c increasing, query u meets a
    better row at every step (every row beats the threshold, every candidate buffer overflows again
    and again); with c decreasing nothing passes after the first k.  Query -u swaps the two."""
    u = unit_rows(rng, 1, E)[0]
    c = np.float32(0.5) + np.arange(N, dtype=np.float32) / np.float32(2 * N)
    assert (np.diff(c) > 0).all()
    if not increasing:
        c = c[::-1].copy()
    return u, (c[:, None] * u[None, :]).astype(np.float32)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("increasing", [True, False])
def test_selection_under_load(increasing, dt):
    rng = np.random.default_rng(33)
    N, E = 3000, 64
    u, g = line_gallery(rng, N, E, increasing)
    q = np.stack([u, -u])
    gr = g if dt == "f32" else ROUND[dt](g)
    want = expected(q, gr, 128, 100.0, 0.0)  # stably sorted: its first 10 columns are the k = 10 result
    # the gallery does what it is meant to (on the f32 rows; bf16 rounding blurs neighbours, the load
    # stays): one query's scores rise strictly along the gallery, the other's fall strictly
    from open_clip_inference.engine import similarity
    L = similarity(q, g, 100.0, 0.0, "logits", 1)
    up, down = (0, 1) if increasing else (1, 0)
    assert (np.diff(L[up]) > 0).all() and (np.diff(L[down]) < 0).all()
    for k in (10, 128):
        wk = (want[0][:, :k], want[1][:, :k])
        for cols in (64, 0):
            try:
                span_cols(cols)
                for r in (1, 2):
                    with route(r):
                        assert_same(search16(q, g, k, dt), wk, f"k {k} span_cols {cols} route {r}")
            finally:
                span_cols(0)


@pytest.mark.parametrize("scale", [100.0, -1.0])
@pytest.mark.parametrize("cols", [64, 0])
def test_ties_on_the_few_query_route(cols, scale):
    rng = np.random.default_rng(15)
    base, g, _ = tied_gallery(rng, 1000)
    q = base[:3] + np.float32(0.25) * unit_rows(rng, 3, 64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    want = expected(q, g, 128, scale, 0.0)
    for r in range(3):
        same = want[1][r][1:] == want[1][r][:-1]
        assert same.sum() >= 100 and (np.diff(want[0][r])[same] > 0).all()
    try:
        span_cols(cols)
        with route(2):
            assert_same(search_once(q, g, 128, scale, 0.0), want)
    finally:
        span_cols(0)


def test_a_nan_query_row_stays_alone():
    """One all-NaN query among five: the others' results are what they are without it, and the NaN row
    (every score NaN: below -inf, by ascending index) returns indices 0 .. k - 1."""
    rng = np.random.default_rng(21)
    k = 10
    g = unit_rows(rng, 500, 64)
    q = unit_rows(rng, 6, 64)
    clean = [0, 1, 3, 4, 5]
    with route(2):
        alone = search_once(q[clean], g, k)
    assert_same(alone, expected(q[clean], g, k, 100.0, 0.0))
    q[2] = np.nan
    for r in (1, 2):
        with route(r):
            idx, score = search_once(q, g, k)
        assert_same((idx[clean], score[clean]), alone, f"route {r}")
        assert np.array_equal(idx[2], np.arange(k)) and np.isnan(score[2]).all()


def test_add_on_one_stream_then_one_query_on_another():
    import torch
    from open_clip_inference import EmbeddingIndex
    rng = np.random.default_rng(5)
    g, q = unit_rows(rng, 264, 64), unit_rows(rng, 1, 64)
    want = expected(q, g, 12, 100.0, 0.0)
    with route(2), EmbeddingIndex(64, 264) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:]).cuda()
            ix.add_device(rest.data_ptr(), 200, s1.cuda_stream)
        with torch.cuda.stream(s2):
            dq = torch.from_numpy(q).cuda()
            di = torch.empty((1, 12), dtype=torch.int64, device="cuda")
            ds = torch.empty((1, 12), dtype=torch.float32, device="cuda")
            ix.search_device(dq.data_ptr(), 1, 12, di.data_ptr(), ds.data_ptr(), 100.0, 0.0, s2.cuda_stream)
            s2.synchronize()
        assert len(ix) == 264
        assert_same((di.cpu().numpy(), ds.cpu().numpy()), want, "search_device after add_device")
