"""Duplicate groups (EmbeddingIndex.duplicate_groups / duplicate_groups_device, Clip.group_duplicates;
csrc/kernels/components.hip) against a dozen lines of numpy over S = logits(rows, rows), the pinned similarity
kernel: the adjacency ok & ok' & (S >= thr) off the diagonal, min-label propagation with pointer jumping until
nothing changes, -1 where ~ok.  Exact: array_equal everywhere.  Shapes: the smallest that reach the path named."""
import functools

import numpy as np
import pytest

from tests.index_cases import ROUND, pattern, span_cols, special_rows, tied_gallery, unit_rows
from tests.index_range_cases import index_of, logits

pytestmark = pytest.mark.gpu


def oracle(S, thr, ok=None):
    """(labels int64 [N], n_groups) from S [N][N]; the pairs i < j decide, as in the self-join."""
    n = len(S)
    ok = np.ones(n, bool) if ok is None else np.asarray(ok, bool)
    with np.errstate(invalid="ignore"):
        A = np.triu(S >= np.float32(thr), 1) & ok[:, None] & ok[None, :]
    A |= A.T
    lab, new = None, np.arange(n)
    while not np.array_equal(new, lab):
        lab = new
        new = np.minimum(lab, np.where(A, lab[None, :], n).min(axis=1))
        new = new[new]  # pointer jumping
    return np.where(ok, lab, -1).astype(np.int64), int((lab == np.arange(n))[ok].sum())


def by_pairs(pairs, n):
    """The components of a pair list: a union-find with the smaller id as the root."""
    parent = list(range(n))
    def find(x):
        while parent[x] != x:
            parent[x] = x = parent[parent[x]]
        return x
    for i, j in pairs:
        a, b = find(int(i)), find(int(j))
        parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], np.int64)


def groups_of(g, thr, scale=1.0, bias=0.0, cols=0, dt="f32", gone=(), **kw):
    """cols: the span cut.  0 and 64 are both one tile per block at these sizes; 192 is blocks of 1 to 3 tiles."""
    span_cols(cols)
    try:
        with index_of(g, dt) as ix:
            if len(gone):
                ix.remove(gone)
            labels, n = ix.duplicate_groups(thr, scale, bias, **kw)
    finally:
        span_cols(0)
    assert labels.dtype == np.int64 and labels.shape == (len(g),) and isinstance(n, int)
    return labels, n


def arc(angles, E=16):
    g = np.zeros((len(angles), E), np.float32)
    g[:, 0], g[:, 1] = np.cos(angles), np.sin(angles)
    return g


def quantile_thr(S, edges):
    off = np.sort(S[np.triu_indices(len(S), 1)])
    return float(off[-min(edges, len(off))]) if len(off) else 0.5


@functools.lru_cache(maxsize=None)
def gallery300():
    g = unit_rows(np.random.default_rng(300), 300, 64)
    return g, logits(g, g, 1.0)


@pytest.mark.parametrize("cols", [0, 64, 192])
@pytest.mark.parametrize("N", [130, 300])
def test_chains(N, cols):
    """Two chains and five isolated rows on an arc, ids permuted: only the transitive closure joins a chain, and a
    chain crosses tiles, panels and spans.  Hooks between blocks decide the result."""
    nA, nB, step = N // 2, N - 5 - N // 2, 0.005
    angles = np.concatenate([np.arange(nA) * step, 1.0 + (nA + np.arange(nB)) * step, 2.6 + 0.1 * np.arange(5)])
    ids = np.random.default_rng(N).permutation(N)  # arc position k is row ids[k]
    g = arc(angles)[np.argsort(ids)]
    S = logits(g, g, 1.0)
    a, b = ids[:nA], ids[nA:nA + nB]
    thr = float(min(S[a[:-1], a[1:]].min(), S[b[:-1], b[1:]].min()))
    assert thr > max(S[a[:-2], a[2:]].max(), S[b[:-2], b[2:]].max())  # S[i, i+1] >= thr > S[i, i+2] along the arc
    labels, n = groups_of(g, thr, cols=cols)
    assert (labels[a] == a.min()).all() and (labels[b] == b.min()).all()
    assert np.array_equal(labels[ids[nA + nB:]], ids[nA + nB:]) and n == 7
    assert np.array_equal(labels, oracle(S, thr)[0])


@pytest.mark.parametrize("cols", [0, 64, 192])
@pytest.mark.parametrize("N", [257, 513])
def test_big_ties(N, cols):
    """Eight distinct rows, N copies: nearly every pair of a tile is a hit."""
    _, g, _ = tied_gallery(np.random.default_rng(N), N)
    _, first, inverse = np.unique(g, axis=0, return_index=True, return_inverse=True)
    labels, n = groups_of(g, 0.99, cols=cols)
    assert np.array_equal(labels, first[inverse.ravel()]) and n == 8


def test_a_cluster_too_large_for_the_pair_list():
    from open_clip_inference.error import ResultOverflow
    g = np.repeat(unit_rows(np.random.default_rng(6), 1, 32), 600, axis=0)
    with index_of(g) as ix:
        with pytest.raises(ResultOverflow):
            ix.duplicates(0.99, max_pairs=1000)  # 179 700 pairs
        assert ix.duplicate_groups(0.99)[1] == 1 and not ix.duplicate_groups(0.99)[0].any()


@pytest.mark.parametrize("scale,bias", [(1.0, 0.0), (100.0, -3.0)])
def test_same_edges_as_duplicates(scale, bias):
    """The threshold AT a score and one ulp above it: the edge set is that of duplicates, bit for bit."""
    g = gallery300()[0]
    thr, seen = quantile_thr(logits(g, g, scale, bias), 50), []
    with index_of(g) as ix:
        for t in (thr, float(np.nextafter(np.float32(thr), np.float32(np.inf)))):
            labels, n = ix.duplicate_groups(t, scale, bias)
            want = by_pairs(ix.duplicates(t, scale, bias)[0], 300)
            assert np.array_equal(labels, want) and n == int((want == np.arange(300)).sum())
            seen.append(labels)
    assert not np.array_equal(seen[0], seen[1])


@pytest.mark.parametrize("N,E,cols", [(N, E, 0) for N in (1, 63, 65, 1000) for E in (16, 80, 512)]
                         + [(1000, E, cols) for E in (16, 80, 512) for cols in (64, 192)])
def test_shapes(N, E, cols):
    """One row (no pair), a ragged panel, a panel of one row, 16 panels (cols = 192: five groups of panels with 1 to
    6 spans, the last group short); a ragged and a multiple k slab."""
    g = unit_rows(np.random.default_rng(N + E), N, E)
    S = logits(g, g, 1.0)
    thr = quantile_thr(S, 40)
    got, want = groups_of(g, thr, cols=cols), oracle(S, thr)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and (N == 1 or got[1] < N)


@pytest.mark.parametrize("cols", [0, 192])
def test_filter_and_removal(cols):
    """Rows 64 .. 127 are filtered out: a panel without a row and (cols = 192) a tile skipped in mid-span."""
    g, S = gallery300()
    thr, gone, allow = quantile_thr(S, 300), np.array([0, 9, 10, 299]), pattern(300)
    allow[64:128] = False
    ok = allow & ~np.isin(np.arange(300), gone)
    labels, n = groups_of(g, thr, cols=cols, gone=gone, allow=allow)
    only, want = groups_of(g[ok], thr, cols=cols), oracle(S, thr, ok)
    assert np.array_equal(labels, want[0]) and n == want[1] and n < ok.sum()
    assert (labels[~ok] == -1).all() and ok[labels[ok]].all()  # a filtered-out row is never a label
    assert np.array_equal(labels[ok], np.flatnonzero(ok)[only[0]]) and n == only[1]
    chain = arc(np.arange(9) * 0.01)  # a chain of nine; without its middle row, two of four
    labels, n = groups_of(chain, 0.9999, gone=[4])
    assert groups_of(chain, 0.9999)[1] == 1 and labels.tolist() == [0, 0, 0, 0, -1, 5, 5, 5, 5] and n == 2


def test_empty_index_and_refusals():
    from open_clip_inference import EmbeddingIndex, _lib
    L, out = _lib.lib(), np.full(5, -7, np.int64)
    lab, cnt = out.ctypes.data, out[4:].ctypes.data
    with EmbeddingIndex(16, 4) as ix:
        labels, n = ix.duplicate_groups(0.5, set_groups=True)
        assert labels.shape == (0,) and n == 0
        assert L.clipgpu_index_components(ix.handle, 0.5, 1.0, 0.0, None, 0, lab, cnt) == 0
        assert out.tolist() == [-7] * 4 + [0]  # no label written, the count zeroed
        for thr, a, b in ((np.nan, lab, cnt), (0.5, None, cnt), (0.5, lab, None)):
            assert L.clipgpu_index_components(ix.handle, thr, 1.0, 0.0, None, 0, a, b) != 0
        for thr, groups in ((np.nan, 1), (0.5, 0)):  # the device form: NaN; no label buffer without to_groups
            assert L.clipgpu_index_components_device(ix.handle, thr, 1.0, 0.0, None, groups, None, None, None) != 0


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_storage_types(dt):
    """A 16-bit index returns what an f32 index of the rounded rows returns; no NaN score is an edge, even at -inf."""
    r = ROUND[dt](gallery300()[0])
    S = logits(r, r, 1.0)
    thr = quantile_thr(S, 100)
    got, ref, want = groups_of(gallery300()[0], thr, dt=dt), groups_of(r, thr), oracle(S, thr)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[0], want[0]) and got[1] == ref[1] == want[1]
    s = ROUND[dt](special_rows())
    S = logits(s, s, 1.0)
    labels, n = groups_of(special_rows(), -np.inf, dt=dt)
    alone = np.isnan(S + np.diag(np.full(len(s), np.nan, np.float32))).all(axis=1)
    assert alone.any() and np.array_equal(labels[alone], np.flatnonzero(alone))
    assert np.array_equal(labels, oracle(S, -np.inf)[0]) and n == oracle(S, -np.inf)[1]


def test_groups_and_device_form():
    import torch
    g, S = gallery300()
    thr, gone, q = quantile_thr(S, 100), [3, 150], unit_rows(np.random.default_rng(5), 5, 64)
    with index_of(g) as ix, index_of(g) as ref:
        ix.remove(gone)
        ref.remove(gone)
        ix.set_groups([3, 7], [1, 1])  # overwritten: every slot's label is
        labels, n = ix.duplicate_groups(thr, set_groups=True)
        assert np.array_equal(ix.groups(), labels) and (labels[gone] == -1).all() and 1 < n < 298
        ref.set_groups(np.flatnonzero(labels >= 0), labels[labels >= 0])
        got, want = ix.search_grouped(q, 10, return_groups=True), ref.search_grouped(q, 10, return_groups=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        s = torch.cuda.Stream()  # not the stream that added the rows
        with torch.cuda.stream(s):
            dl = torch.full((300 + 64,), -7, dtype=torch.int32, device="cuda")
            dc = torch.full((2,), -7, dtype=torch.int32, device="cuda")
            ix.duplicate_groups_device(thr, dl.data_ptr(), dc.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
        assert np.array_equal(dl.cpu().numpy(), np.r_[labels, [-7] * 64]) and dc.cpu().tolist() == [n, -7]


def test_clip_group_duplicates():
    """The facade on the seeded tiny model with one image repeated, against duplicate_groups."""
    from open_clip_inference import Clip
    from tests.helpers import cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims = images()
    with clip.build_index(list(ims) + [ims[0]]) as index:
        labels, groups = index.duplicate_groups(0.999)[0], clip.group_duplicates(index, 0.999)
        assert [0, len(index) - 1] in groups
        assert groups == [np.flatnonzero(labels == l).tolist() for l in np.unique(labels) if (labels == l).sum() > 1]
        assert clip.group_duplicates(index, 0.999, apply=True) == groups and np.array_equal(index.groups(), labels)
