"""Filtered search of the embedding index (EmbeddingIndex.search(..., allow=), the MASKED phase-1 kernels
of csrc/kernels/topk.hip) on the GPU.

Oracle: for a gallery g, queries q and an allowed set A (ascending ids), the filtered result equals, bit
for bit, the existing unfiltered search of an index holding g[A], with its indices mapped through A and
(-1, -inf) past min(k, |A|): score bits do not depend on a row's position, and ascending-index tie order
survives a monotone map.  The cases without NaN are also checked against similarity(..., "logits") with a
stable argsort over the allowed columns.  Indices are compared with == and scores as uint32 views: there
is no tolerance anywhere."""
import functools

import numpy as np
import pytest

from tests.index_cases import assert_same, logits_oracle, padding, route, span_cols, tied_gallery, unit_rows

pytestmark = pytest.mark.gpu

SCALE, BIAS = 100.0, 0.0


def sub_index_oracle(q, g, allow, k, dt="f32", scale=SCALE, bias=BIAS):
    """The unfiltered search of an index that holds only the allowed rows, indices mapped back."""
    from open_clip_inference import EmbeddingIndex
    A = np.flatnonzero(allow)
    if len(A) == 0:
        return padding(len(q), k)
    with EmbeddingIndex(g.shape[1], len(A), dtype=dt) as ix:
        ix.add(g[A])
        idx, score = ix.search(q, k, scale, bias)
    return np.where(idx >= 0, A[np.maximum(idx, 0)], -1).astype(np.int64), score


@functools.lru_cache(maxsize=None)
def data(N, E=64, Q=5):
    """Gallery, queries and their logits matrix for one N: computed once, shared, never written to."""
    from open_clip_inference.engine import similarity
    rng = np.random.default_rng(7000 + N + E)
    g, q = unit_rows(rng, N, E), unit_rows(rng, Q, E)
    L = similarity(q, g, SCALE, BIAS, "logits", 1)
    for a in (g, q, L):
        a.setflags(write=False)
    return g, q, L


def masks(N, L):
    """name -> (allow, k).  Columns at the edges of mask words (31 | 32), of the few-query kernel's tiles
    (15 | 16), of the wide kernel's tiles and of 64-column spans (63 | 64), and the last row."""
    out = {}
    out["all"] = (np.ones(N, bool), 10)
    out["none"] = (np.zeros(N, bool), 10)
    for c in sorted({0, 15, 16, 31, 32, 63, 64, N - 1}):
        if c < N:
            m = np.zeros(N, bool)
            m[c] = True
            out[f"only {c}"] = (m, 10)
    out["alternating"] = (np.arange(N) % 2 == 1, 10)
    m = np.zeros(N, bool)  # one 64-column span (the second where there is one): the others are empty
    m[64:128] = True
    if N <= 64:
        m[N // 2:] = True
    out["one span"] = (m, 10)
    m = np.ones(N, bool)  # a 64-column tile of zeros between allowed tiles
    m[64:128] = False
    out["empty tile"] = (m, 10)
    m = np.zeros(N, bool)
    m[N // 4: N // 4 + (N + 1) // 2] = True
    out["range"] = (m, 10)
    m = np.ones(N, bool)  # the three best rows of every query
    m[np.argsort(-L, axis=1, kind="stable")[:, :3].ravel()] = False
    out["best rows out"] = (m, 10)
    m = np.zeros(N, bool)  # fewer allowed rows than k
    m[[0, N // 2, N - 1]] = True
    out["3 rows k 10"] = (m, 10)
    out["3 rows k 128"] = (m, 128)
    m = np.ones(N, bool)
    m[N // 3] = False
    out["N - 1 rows k 128"] = (m, 128)
    return out


# cols 256 is one span of four tiles at N = 200: the only cut at which the wide kernel skips a tile
# inside a span it works on (the default cut and 64 make every tile a span of its own at these N)
@pytest.mark.parametrize("cols", [64, 0, 256])
@pytest.mark.parametrize("r", [1, 2], ids=["wide", "few-query"])
@pytest.mark.parametrize("N", [1, 50, 129, 200])
def test_masks(N, r, cols):
    from open_clip_inference import EmbeddingIndex
    g, q, L = data(N)
    try:
        span_cols(cols)
        with route(r), EmbeddingIndex(64, N) as ix:
            ix.add(g)
            unfiltered = {k: ix.search(q, k, SCALE, BIAS) for k in (10, 128)}
            for name, (allow, k) in masks(N, L).items():
                got = ix.search(q, k, SCALE, BIAS, allow=allow)
                what = f"N {N} route {r} span_cols {cols} mask {name}"
                assert_same(got, sub_index_oracle(q, g, allow, k), what)
                assert_same(got, logits_oracle(L, allow, k), what + " (logits)")
                n = min(k, int(allow.sum()))
                assert (got[0][:, :n] >= 0).all() and allow[got[0][:, :n]].all(), what
                assert (got[0][:, n:] == -1).all() and np.isneginf(got[1][:, n:]).all(), what
                if name == "all":
                    assert_same(got, unfiltered[k], what + " vs unfiltered")
            assert_same(ix.search(q, 10, SCALE, BIAS), unfiltered[10], "the unfiltered search is unchanged")
    finally:
        span_cols(0)


def search_words(ix, q, k, words):
    """clipgpu_index_search_filtered with the caller's own bitmap words."""
    from open_clip_inference import _lib
    idx = np.empty((len(q), k), np.int64)
    score = np.empty((len(q), k), np.float32)
    _lib.check(_lib.lib().clipgpu_index_search_filtered(ix.handle, q.ctypes.data, len(q), k, SCALE, BIAS,
                                                        words.ctypes.data, idx.ctypes.data, score.ctypes.data))
    return idx, score


@pytest.mark.parametrize("r", [1, 2], ids=["wide", "few-query"])
def test_bits_past_the_size_are_ignored(r):
    """N = 50: bits 50 .. 63 of the caller's last word are garbage and change nothing; the bitmap sits at
    an address that is 4- but not 8-byte aligned, and the words behind it are never read as allowed rows."""
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.index import pack_allow
    N = 50
    g, q, L = data(N)
    allow = np.arange(N) % 3 != 0
    buf = np.full(8, 0xFFFFFFFF, np.uint32)
    words = buf[1:3]  # 4-byte aligned only
    assert words.ctypes.data % 8 == 4
    words[:] = pack_allow(allow)
    words[1] |= np.uint32(0xFFFFFFFF << (N - 32) & 0xFFFFFFFF)
    assert (int(words[1]) >> (N - 32)) == (1 << (64 - N)) - 1
    with route(r), EmbeddingIndex(64, 64) as ix:  # capacity 64: rows 50 .. 63 are slots without a row
        ix.add(g)
        for k in (10, 128):
            got = search_words(ix, q, k, words)
            assert_same(got, ix.search(q, k, SCALE, BIAS, allow=allow), f"k {k} vs clean bits")
            assert_same(got, logits_oracle(L, allow, k), f"k {k}")
            assert got[0].max() < N


@pytest.mark.parametrize("cols", [64, 0])
@pytest.mark.parametrize("r", [1, 2], ids=["wide", "few-query"])
def test_ties_under_a_mask_come_out_by_ascending_original_index(r, cols):
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    rng = np.random.default_rng(15)
    base, g, _ = tied_gallery(rng, 300)
    q = base[:3] + np.float32(0.25) * unit_rows(rng, 3, 64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    allow = rng.random(300) < 0.6
    L = similarity(q, g, SCALE, BIAS, "logits", 1)
    want = logits_oracle(L, allow, 128)
    for row in range(3):  # long runs of equal scores, ascending original indices within each
        same = want[1][row][1:] == want[1][row][:-1]
        assert same.sum() >= 80 and (np.diff(want[0][row])[same] > 0).all()
    try:
        span_cols(cols)
        with route(r), EmbeddingIndex(64, 300) as ix:
            ix.add(g)
            got = ix.search(q, 128, SCALE, BIAS, allow=allow)
        assert_same(got, want)
        with route(r):
            assert_same(got, sub_index_oracle(q, g, allow, 128))
    finally:
        span_cols(0)


@pytest.mark.parametrize("r", [1, 2], ids=["wide", "few-query"])
def test_a_nan_row_is_an_entry_and_a_disallowed_row_is_not(r):
    """Row 5 is NaN (every score NaN: below -inf), rows 3 and 9 score -inf for every query.  Allowed, the
    NaN row comes last, after the -inf rows, once k exceeds the rest; disallowed, a row never appears."""
    from open_clip_inference import EmbeddingIndex
    N = 20
    rng = np.random.default_rng(3)
    g, q = unit_rows(rng, N, 64), unit_rows(rng, 4, 64)
    q[:, 0] = np.abs(q[:, 0]) + np.float32(0.1)
    g[5] = np.nan
    for j in (3, 9):
        g[j] = 0
        g[j, 0] = -np.inf
    with route(r), EmbeddingIndex(64, N) as ix:
        ix.add(g)
        every = np.ones(N, bool)
        idx, score = ix.search(q, N, SCALE, BIAS, allow=every)
        assert_same((idx, score), sub_index_oracle(q, g, every, N))
        assert (idx[:, -3:] == [3, 9, 5]).all()
        assert np.isneginf(score[:, -3:-1]).all() and np.isnan(score[:, -1]).all()
        assert np.isfinite(score[:, :-3]).all()
        for out in ([5], [3], [3, 5, 9], [0, 5]):
            allow = every.copy()
            allow[out] = False
            idx, score = ix.search(q, N, SCALE, BIAS, allow=allow)
            assert_same((idx, score), sub_index_oracle(q, g, allow, N), f"without {out}")
            assert not np.isin(idx, out).any()
            assert (idx[:, N - len(out):] == -1).all() and np.isneginf(score[:, N - len(out):]).all()
            kept = [j for j in (3, 9, 5) if j not in out]  # the tail of what is left, in this order
            assert (idx[:, N - len(out) - len(kept): N - len(out)] == kept).all()


@pytest.mark.parametrize("dt,E", [("f16", 64), ("bf16", 64), ("f32", 48)])
def test_storage_types_and_a_short_last_slab(dt, E):
    from open_clip_inference import EmbeddingIndex
    N = 200
    g, q, _ = data(N, E)
    rng = np.random.default_rng(E)
    allow = rng.random(N) < 0.5
    allow[64:128] = False
    try:
        for cols in (64, 0):
            span_cols(cols)
            for r in (1, 2):
                with route(r), EmbeddingIndex(E, N, dtype=dt) as ix:
                    ix.add(g)
                    got = ix.search(q, 10, SCALE, BIAS, allow=allow)
                    assert_same(got, sub_index_oracle(q, g, allow, 10, dt), f"{dt} route {r} span_cols {cols}")
    finally:
        span_cols(0)


def test_257_queries_share_one_mask():
    """One wide chunk of 256 rows and one few-query chunk of one row (default routes), one filter for both."""
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    N = 200
    g, _, _ = data(N)
    rng = np.random.default_rng(257)
    q = unit_rows(rng, 257, 64)
    allow = rng.random(N) < 0.3
    L = similarity(q, g, SCALE, BIAS, "logits", 1)
    with EmbeddingIndex(64, N) as ix:
        ix.add(g)
        got = ix.search(q, 10, SCALE, BIAS, allow=allow)
    assert_same(got, logits_oracle(L, allow, 10))
    assert_same(got, sub_index_oracle(q, g, allow, 10))


def test_17_queries_take_the_wide_kernel_by_default():
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    N = 129
    g, _, _ = data(N)
    rng = np.random.default_rng(17)
    q = unit_rows(rng, 17, 64)
    allow = np.arange(N) % 5 != 2
    with EmbeddingIndex(64, N) as ix:
        ix.add(g)
        got = ix.search(q, 10, SCALE, BIAS, allow=allow)
    assert_same(got, logits_oracle(similarity(q, g, SCALE, BIAS, "logits", 1), allow, 10))


def test_add_on_one_stream_then_a_filtered_query_on_another():
    import torch
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    from open_clip_inference.index import pack_allow
    rng = np.random.default_rng(5)
    g, q = unit_rows(rng, 264, 64), unit_rows(rng, 1, 64)
    allow = rng.random(264) < 0.5
    want = logits_oracle(similarity(q, g, SCALE, BIAS, "logits", 1), allow, 12)
    with route(2), EmbeddingIndex(64, 264) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:]).cuda()
            ix.add_device(rest.data_ptr(), 200, s1.cuda_stream)
        with torch.cuda.stream(s2):
            dq = torch.from_numpy(q).cuda()
            da = torch.from_numpy(pack_allow(allow).view(np.int32)).cuda()
            di = torch.empty((1, 12), dtype=torch.int64, device="cuda")
            ds = torch.empty((1, 12), dtype=torch.float32, device="cuda")
            ix.search_device(dq.data_ptr(), 1, 12, di.data_ptr(), ds.data_ptr(), SCALE, BIAS, s2.cuda_stream,
                             d_allow=da.data_ptr())
            s2.synchronize()
        assert len(ix) == 264
        assert_same((di.cpu().numpy(), ds.cpu().numpy()), want, "search_device with d_allow after add_device")
