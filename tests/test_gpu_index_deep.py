"""The deep search (EmbeddingIndex.search_deep, 1 <= k <= 4096) against the stable descending sort of the full
logits matrix: exact, indices by array_equal and scores on their uint32 views.  Shapes are the smallest that
reach the path named beside them."""
import numpy as np
import pytest

from tests.index_cases import (ROUND, assert_same, bits_equal_with_nans, logits_oracle, pattern, route, routes_for,
                               span_cols, special_rows, tied_gallery, unit_rows)
from tests.index_range_cases import index_of, logits

pytestmark = pytest.mark.gpu


def deep_cand(n):
    from open_clip_inference import _lib
    _lib.check(_lib.lib().clipgpu_test_deep_cand(n))


def expected_passes(L, k, cand=8192):
    """The select's rule on the keys themselves (finite scores, no -0; every row live and allowed): the first
    digit d, 8 bits each from the top of (monotone score bits << 32 | ~row), at which the keys at or above the
    bucket of the k-th largest are at most `cand`."""
    b = np.ascontiguousarray(L, np.float32).view(np.uint32).astype(np.uint64)
    mono = np.where(b >> np.uint64(31), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    keys = (mono << np.uint64(32)) | (~np.arange(L.shape[1], dtype=np.uint32)).astype(np.uint64)
    kth = np.sort(keys, axis=1)[:, -k]
    shifts = [np.uint64(64 - 8 * d) for d in range(1, 9)]
    return np.array([1 + next(i for i, s in enumerate(shifts) if (row >> s >= t >> s).sum() <= cand)
                     for row, t in zip(keys, kth)])


def check(ix, q, L, ok, k, **kw):
    """search_deep on every route the query count allows against the oracle; returns the last pass counts."""
    want = logits_oracle(L, ok, k)
    for r in routes_for(len(q)):
        with route(r):
            idx, score, passes = ix.search_deep(q, k, 100.0, 0.0, return_passes=True, **kw)
        assert_same((idx, score), want, f"route {r}")
        assert passes.dtype == np.int32 and ((1 <= passes) & (passes <= 8)).all()
    return passes


@pytest.mark.parametrize("Q,N,E,k,cols", [
    (1, 200, 16, 129, 0),       # the first k above the old cap
    (3, 1000, 80, 1000, 0),     # k = N, ragged E
    (3, 1000, 80, 1000, 64),    # ... and one 64-column tile per span
    (3, 100, 64, 500, 0),       # k > N: padding, fewer keys than k
    (16, 5000, 64, 4096, 0),    # the cap
    (17, 5000, 64, 300, 0),     # the wide route
    (70, 4097, 512, 2048, 0),   # two query tiles, several slabs, N one past a tile
    (257, 300, 64, 200, 0),     # a 256-row chunk and a one-row few-query chunk
])
def test_shapes(Q, N, E, k, cols):
    rng = np.random.default_rng(Q * 1000 + k)
    g, q = unit_rows(rng, N, E), unit_rows(rng, Q, E)
    span_cols(cols)
    try:
        with index_of(g) as ix:
            check(ix, q, logits(q, g), np.ones(N, bool), k)
    finally:
        span_cols(0)


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("special", [False, True])
def test_agrees_with_search(k, special):
    """Up to the search's cap the deep search is the search, bit for bit -- also over +-0, +-inf, NaN and
    subnormal scores."""
    rng = np.random.default_rng(k)
    g = special_rows() if special else unit_rows(rng, 300, 64)
    q = np.concatenate([unit_rows(rng, 3, g.shape[1]), np.zeros((1, g.shape[1]), np.float32), g[:2]])
    with index_of(g) as ix:
        want = ix.search(q, k)
        for r in routes_for(len(q)):
            with route(r):
                got = ix.search_deep(q, k)
            assert np.array_equal(got[0], want[0]), r
            bits_equal_with_nans(got[1], want[1])


@pytest.mark.parametrize("cand", [0, 1])
def test_tied_scores(cand):
    """Eight distinct rows repeated: every score is shared by hundreds of rows.  With a candidate capacity of
    k the select has to resolve the k-th key itself, through all eight digits (unless a bucket of an earlier
    digit happens to end at the k-th key: not with this seed, and expected_passes would say so)."""
    rng = np.random.default_rng(11)
    base, g, _ = tied_gallery(rng, 3000, 64)
    q = np.concatenate([base[:2], unit_rows(rng, 1, 64)])
    L = logits(q, g)
    deep_cand(cand)
    try:
        with index_of(g) as ix:
            passes = check(ix, q, L, np.ones(3000, bool), 1000)
    finally:
        deep_cand(0)
    assert np.array_equal(passes, expected_passes(L, 1000, 1000 if cand else 8192))
    if cand == 1:
        assert (passes == 8).all()


def test_identical_rows_pass_count():
    """The four score digits cannot split 10,000 equal scores below the capacity of 8192, nor can the first two
    digits of ~row (all ones below row 65536); the third leaves rows 0 .. 255 in the k-th key's bucket: 7."""
    N, k = 10000, 200
    rng = np.random.default_rng(6)
    g = np.repeat(unit_rows(rng, 1, 16), N, axis=0)
    q = unit_rows(rng, 2, 16)
    L = logits(q, g)
    derived = expected_passes(L, k)
    assert (derived == 7).all()
    with index_of(g) as ix:
        idx, score, passes = ix.search_deep(q, k, 100.0, 0.0, return_passes=True)
    assert np.array_equal(idx, np.tile(np.arange(k), (2, 1)))
    assert np.array_equal(score.view(np.uint32), L[:, :k].view(np.uint32))
    assert np.array_equal(passes, derived)


def test_no_mass_ties_few_passes():
    rng = np.random.default_rng(7)
    g, q = unit_rows(rng, 2000, 64), unit_rows(rng, 3, 64)
    with index_of(g) as ix:
        assert (check(ix, q, logits(q, g), np.ones(2000, bool), 300) <= 4).all()


@pytest.mark.parametrize("k", [300, 500])  # fewer, and more, than the rows that stay allowed
def test_filter_and_removal(k):
    rng = np.random.default_rng(8)
    N = 1000
    g, q = unit_rows(rng, N, 64), unit_rows(rng, 3, 64)
    allow, dead = pattern(N), rng.choice(N, 50, replace=False)
    ok = allow.copy()
    ok[dead] = False
    assert 300 < ok.sum() < 500
    with index_of(g) as ix:
        ix.remove(dead)
        check(ix, q, logits(q, g), ok, k, allow=allow)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_storage_types(dt):
    rng = np.random.default_rng(9)
    g, q = unit_rows(rng, 1000, 64), unit_rows(rng, 3, 64)
    with index_of(g, dt) as ix:
        check(ix, q, logits(q, ROUND[dt](g)), np.ones(1000, bool), 300)


def test_device_form_follows_an_add_on_another_stream():
    import torch
    from open_clip_inference import EmbeddingIndex
    rng = np.random.default_rng(10)
    g, q, k = unit_rows(rng, 1000, 64), unit_rows(rng, 5, 64), 300
    with EmbeddingIndex(64, 1000) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:]).cuda()
            ix.add_device(rest.data_ptr(), 936, s1.cuda_stream)
        with torch.cuda.stream(s2):
            dq = torch.from_numpy(q).cuda()
            di = torch.full((5, k), -7, dtype=torch.int64, device="cuda")
            ds = torch.zeros((5, k), dtype=torch.float32, device="cuda")
            dp = torch.zeros(5, dtype=torch.int32, device="cuda")
            ix.search_deep_device(dq.data_ptr(), 5, k, di.data_ptr(), ds.data_ptr(), 100.0, 0.0, s2.cuda_stream,
                                  d_passes=dp.data_ptr())
            s2.synchronize()
        idx, score, passes = ix.search_deep(q, k, 100.0, 0.0, return_passes=True)
        assert_same((di.cpu().numpy(), ds.cpu().numpy()), (idx, score))
        assert np.array_equal(dp.cpu().numpy(), passes)
        assert_same((idx, score), logits_oracle(logits(q, g), np.ones(1000, bool), k))


def test_work_area_outlives_the_codes():
    """The deep search's work area belongs to the handle, not to the codes: dropping the codes leaves it alone."""
    rng = np.random.default_rng(12)
    g, q = unit_rows(rng, 1000, 64), unit_rows(rng, 3, 64)
    with index_of(g) as ix:
        first = ix.search_deep(q, 300, 100.0)
        ix.enable_codes()
        ix.drop_codes()
        assert_same(ix.search_deep(q, 300, 100.0), first)
        ix.enable_codes()
        ix.drop_codes()
        assert_same(first, logits_oracle(logits(q, g), np.ones(1000, bool), 300))


def test_errors():
    from open_clip_inference import DEEP_K_MAX, EmbeddingIndex, _lib
    assert DEEP_K_MAX == 4096
    q = np.zeros((1, 16), np.float32)
    out = np.zeros(8192, np.int64)
    with EmbeddingIndex(16, 8) as ix:
        for k in (0, -1, 4097):
            with pytest.raises(ValueError, match=r"1\.\.4096"):
                ix.search_deep(q, k)
            assert _lib.lib().clipgpu_index_search_deep(ix.handle, q.ctypes.data, 1, k, 1.0, 0.0, None, out.ctypes.data,
                                                        out.ctypes.data, None) == 1
            assert b"1..4096" in _lib.lib().clipgpu_last_error()
        with pytest.raises(Exception, match="Empty batch"):
            ix.search_deep(q, 200)
        ix.add(q)
        with pytest.raises(Exception, match="128"):
            ix.search(q, 129)
