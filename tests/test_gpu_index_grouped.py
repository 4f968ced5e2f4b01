"""Grouped search (EmbeddingIndex.set_groups / groups / search_grouped / search_grouped_device, Clip.search_grouped;
csrc/kernels/grouped.hip) against a few lines of numpy over the full logits matrix: the allowed live columns in
stable descending order, the first occurrence of each label, cut to k.  Exact: indices and groups by array_equal,
scores on their uint32 views.  Shapes are the smallest that reach the path named beside them."""
from contextlib import contextmanager

import numpy as np
import pytest

from tests.index_cases import ROUND, assert_same, pattern, span_cols, special_rows, tied_gallery, unit_rows
from tests.index_range_cases import index_of, logits

pytestmark = pytest.mark.gpu


@contextmanager
def collapse(mode):
    from open_clip_inference import _lib
    _lib.check(_lib.lib().clipgpu_test_grouped_collapse(mode))
    try:
        yield
    finally:
        _lib.check(_lib.lib().clipgpu_test_grouped_collapse(0))


def runs(n, length):
    return np.arange(n) // length


def mixed(n):
    """Half the rows ungrouped (-1), the rest in runs of 3."""
    lab = np.arange(n) // 3
    lab[np.arange(n) % 2 == 0] = -1
    return lab


def oracle(L, labels, ok, k):
    """(idx, score, group) from the logits matrix L [Q][N]; labels int [N], -1 = ungrouped; ok bool [N]."""
    own = np.where(labels < 0, -1 - np.arange(len(labels)), labels)  # an ungrouped row: a group of its own
    A = np.flatnonzero(ok)
    idx = np.full((len(L), k), -1, np.int64)
    score = np.full((len(L), k), -np.inf, np.float32)
    group = np.full((len(L), k), -1, np.int64)
    for q, row in enumerate(L):
        cols = A[np.argsort(-row[A], kind="stable")]
        _, first = np.unique(own[cols], return_index=True)
        reps = cols[np.sort(first)][:k]
        idx[q, :len(reps)], score[q, :len(reps)], group[q, :len(reps)] = reps, row[reps], labels[reps]
    return idx, score, group


def check(ix, q, L, labels, ok, k, what="", **kw):
    """Both forms of phase 1 against the oracle."""
    want = oracle(L, labels, ok, k)
    for mode in (1, 2):
        with collapse(mode):
            got = ix.search_grouped(q, k, 100.0, 0.0, return_groups=True, **kw)
        assert_same(got, want, (what, mode))
        assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2]), (what, mode)


def labelled(g, labels, dt="f32"):
    ix = index_of(g, dt)
    ids = np.flatnonzero(labels >= 0)
    if len(ids):
        ix.set_groups(ids, labels[ids])
    return ix


@pytest.mark.parametrize("Q,N,E,k,labeling,cols", [
    (1, 200, 16, 10, lambda n: runs(n, 4), 0),        # the smallest
    (5, 300, 64, 16, lambda n: runs(n, 5), 0),        # runs that straddle 16-column tiles
    (16, 1000, 80, 128, lambda n: runs(n, 48), 64),   # ... and spans: the merge's kill pass, the cap of k, a ragged slab
    (3, 1000, 64, 16, lambda n: np.arange(n) % 7, 0),  # fewer groups than k: padding, a threshold that stays 0
    (40, 4097, 512, 32, lambda n: np.arange(n) % 300, 0),  # three query tiles, scattered labels, N past a tile
    (17, 300, 64, 64, mixed, 0),                      # half the rows ungrouped, the rest in runs of 3
])
def test_shapes(Q, N, E, k, labeling, cols):
    rng = np.random.default_rng(Q * 1000 + k)
    g, q, labels = unit_rows(rng, N, E), unit_rows(rng, Q, E), labeling(N)
    span_cols(cols)
    try:
        with labelled(g, labels) as ix:
            check(ix, q, logits(q, g), labels, np.ones(N, bool), k)
    finally:
        span_cols(0)


@pytest.mark.parametrize("k", [10, 128])
def test_an_ungrouped_index_is_the_search(k):
    rng = np.random.default_rng(3)
    g, q = unit_rows(rng, 1000, 64), unit_rows(rng, 20, 64)
    with index_of(g) as ix:
        want = ix.search(q, k, 100.0)
        for mode in (1, 2):
            with collapse(mode):
                idx, score, group = ix.search_grouped(q, k, 100.0, return_groups=True)
            assert_same((idx, score), want, mode)
            assert (group == -1).all()


@pytest.mark.parametrize("labeling", [lambda n: runs(n, 16), lambda n: np.arange(n) % 11])
def test_ties(labeling):
    """Eight distinct rows repeated: hundreds of rows share a score.  A group's representative is its lowest tied
    row, and groups with equal best scores come out by ascending representative."""
    rng = np.random.default_rng(11)
    base, g, _ = tied_gallery(rng, 3000, 64)
    labels = labeling(3000)
    with labelled(g, labels) as ix:
        check(ix, base, logits(base, g), labels, np.ones(3000, bool), 128)


def test_special_values():
    """Two rows per group over scores of +-0, +-inf, NaN and subnormals: a NaN ranks below -inf, a group of only
    NaN rows is still a group, and the zeros keep their own bits."""
    s = special_rows()
    g = np.concatenate([s[:3], s[2:]])  # the row with the infinities and NaNs twice: rows 2 and 3, one group
    N, E = g.shape
    q = np.concatenate([unit_rows(np.random.default_rng(12), 3, E), np.zeros((1, E), np.float32), g[6:8]])
    L = logits(q, g)
    labels = runs(N, 2)
    assert np.isnan(L[:, 2:4]).all() and (L == 0).any()
    with labelled(g, labels) as ix:
        check(ix, q, L, labels, np.ones(N, bool), N)


@pytest.mark.parametrize("k", [20, 128])  # fewer, and more, than the groups that are left
def test_filter_and_removal(k):
    """pattern(N) as the filter, and the current representative of several groups removed: the next best row of
    each takes its place."""
    rng = np.random.default_rng(8)
    N, labels = 300, runs(300, 6)
    g, q = unit_rows(rng, N, 64), unit_rows(rng, 4, 64)
    L, allow = logits(q, g), pattern(N)
    reps = np.unique(oracle(L, labels, allow, 8)[0])
    ok = allow.copy()
    ok[reps] = False
    assert 20 < len(np.unique(labels[ok])) < 128
    with labelled(g, labels) as ix:
        check(ix, q, L, labels, allow, k, "filter", allow=allow)
        ix.remove(reps)
        check(ix, q, L, labels, ok, k, "removal", allow=allow)
        assert not np.isin(ix.search_grouped(q, k, 100.0, allow=allow)[0], reps).any()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_storage_types(dt):
    rng = np.random.default_rng(9)
    g, q, labels = unit_rows(rng, 1000, 64), unit_rows(rng, 5, 64), runs(1000, 7)
    with labelled(g, labels, dt) as ix:
        check(ix, q, logits(q, ROUND[dt](g)), labels, np.ones(1000, bool), 40)


def test_label_state():
    from open_clip_inference import EmbeddingIndex
    rng = np.random.default_rng(13)
    g, q = unit_rows(rng, 200, 64), unit_rows(rng, 3, 64)
    every = np.ones(200, bool)
    with EmbeddingIndex(64, 256) as ix:
        ix.add(g[:100])
        assert (ix.groups() == -1).all()  # before anything is allocated
        labels = np.full(200, -1)
        labels[:100] = runs(100, 4)
        ix.set_groups(np.arange(100), labels[:100])  # after add
        ix.add(g[100:])  # new rows are ungrouped
        assert np.array_equal(ix.groups(), labels) and ix.groups().dtype == np.int64
        check(ix, q, logits(q, g), labels, every, 30, "set after add")
        labels[[5, 150, 151]] = [2**31 - 1, 7, 7]  # relabelling, the largest label, a late row into an old group
        labels[[0, 1]] = -1  # back to ungrouped
        ix.set_groups([5, 150, 151, 0, 1], labels[[5, 150, 151, 0, 1]])
        assert np.array_equal(ix.groups(), labels)
        check(ix, q, logits(q, g), labels, every, 30, "relabelled")
        g2 = g.copy()
        g2[[8, 150]] = unit_rows(rng, 2, 64)
        ix.set_rows([8, 150], g2[[8, 150]])  # keeps the labels
        assert np.array_equal(ix.groups(), labels)
        check(ix, q, logits(q, g2), labels, every, 30, "set_rows")
        ix.clear()
        ix.add(g)
        assert (ix.groups() == -1).all()
        assert_same(ix.search_grouped(q, 30, 100.0), ix.search(q, 30, 100.0), "cleared")


def test_device_form_follows_an_add_on_another_stream():
    import torch
    from open_clip_inference import EmbeddingIndex
    rng = np.random.default_rng(10)
    Q, k = 5, 20
    g, q, labels = unit_rows(rng, 1000, 64), unit_rows(rng, Q, 64), runs(1000, 9)
    with EmbeddingIndex(64, 1000) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:]).cuda()
            ix.add_device(rest.data_ptr(), 936, s1.cuda_stream)
        ix.set_groups(np.arange(1000), labels)
        with torch.cuda.stream(s2):
            dq = torch.from_numpy(q).cuda()
            di = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
            dg = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
            ds = torch.zeros((Q, k), dtype=torch.float32, device="cuda")
            ix.search_grouped_device(dq.data_ptr(), Q, k, di.data_ptr(), ds.data_ptr(), 100.0, 0.0, s2.cuda_stream,
                                     d_group=dg.data_ptr())
            s2.synchronize()
        want = oracle(logits(q, g), labels, np.ones(1000, bool), k)
        assert_same((di.cpu().numpy(), ds.cpu().numpy()), want)
        assert np.array_equal(dg.cpu().numpy(), want[2])


def test_errors():
    from open_clip_inference import EmbeddingIndex, _lib
    L = _lib.lib()
    t = np.zeros((4, 16), np.float32)
    out = np.zeros(4096, np.int64)

    def raw_search(k):
        rc = L.clipgpu_index_search_grouped(ix.handle, t.ctypes.data, 1, k, 1.0, 0.0, None, out.ctypes.data,
                                            out.ctypes.data, None)
        return rc, L.clipgpu_last_error()

    def raw_set(ids, groups):
        i, g = np.asarray(ids, np.int64), np.asarray(groups, np.int32)
        return L.clipgpu_index_set_groups(ix.handle, i.ctypes.data, g.ctypes.data, len(i)), L.clipgpu_last_error()

    with EmbeddingIndex(16, 8) as ix:
        with pytest.raises(Exception, match="Empty batch"):
            ix.search_grouped(t[:1], 1)
        rc, err = raw_search(1)
        assert rc == 1 and b"Empty batch" in err
        ix.add(t)
        for k in (0, 129):
            with pytest.raises(ValueError, match=r"1\.\.128"):
                ix.search_grouped(t[:1], k)
            rc, err = raw_search(k)
            assert rc == 1 and b"1..128" in err, err
        with pytest.raises(Exception, match="Shape error"):
            ix.search_grouped(np.zeros((1, 32), np.float32), 1)
        with pytest.raises(Exception, match="out of range"):
            ix.set_groups([4], [0])
        with pytest.raises(ValueError, match=r"0\.\.2147483647"):
            ix.set_groups([0], [-2])
        for args, msg in ((([4], [0]), b"id out of range"), (([-1], [0]), b"id out of range"),
                          (([0], [-2]), b"0..2147483647"), (([1, 1], [0, 0]), b"duplicate id")):
            rc, err = raw_set(*args)
            assert rc == 1 and msg in err, (args, err)
        assert (ix.groups() == -1).all()  # the refused calls changed nothing
        assert raw_search(1)[0] == 0 and raw_set([0, 3], [5, -1])[0] == 0
        assert list(ix.groups()) == [5, -1, -1, -1]


def test_clip_search_grouped():
    """The facade on the seeded tiny model, against index.search_grouped of the same embeddings."""
    from open_clip_inference import Clip
    from tests.helpers import TEXTS, cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    imgs = images()
    labels = np.arange(len(imgs)) // 2
    scale, bias = clip._scale_bias()
    with clip.build_index(imgs, groups=labels) as index:
        assert np.array_equal(index.groups(), labels)
        idx, score, group = index.search_grouped(clip.text.embed_texts(TEXTS), 3, float(scale), float(bias),
                                                 return_groups=True)
        want = [[(int(i), float(s), int(g)) for i, s, g in zip(ri, rs, rg) if i >= 0]
                for ri, rs, rg in zip(idx, score, group)]
        got = clip.search_grouped(index, TEXTS, 3)
        assert got == want and all(len({g for _, _, g in r}) == len(r) > 0 for r in got)
