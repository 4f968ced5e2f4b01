"""The embedding index's assignment and k-means on the GPU (EmbeddingIndex.assign, assign_device, kmeans, rows_at,
Clip.cluster; csrc/kernels/cluster.hip), against the oracles of tests/index_cluster_cases.py.

assign: labels and scores from assign_oracle(similarity(centroids, rows as stored, "logits")), which is pinned
bit-equal to the search.  kmeans: every field from lloyd(..., logits_fn=similarity), the update restated in numpy.
Every comparison is exact: labels and counts with array_equal, scores, centroids and sums on their integer views.
tests/test_cpu_index_cluster.py shows that each assertion here catches the matching mutant of its oracle."""
import numpy as np
import pytest

from tests import index_cluster_cases as cases
from tests.index_cases import ROUND, pattern, span_cols, tied_gallery, unit_rows

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
CS = (1, 15, 17, 64, 65, 130)  # the 16- and 64-row tile seams on the centroid side


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- assign ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 65, 1000])
@pytest.mark.parametrize("E", [16, 80, 512])
def test_assign_shapes(E, N):
    """E: one short slab; 64 + 16; eight slabs.  N around the 64-row tile and 16 blocks."""
    rng = np.random.default_rng(1000 * E + N)
    g, cen = unit_rows(rng, N, E), unit_rows(rng, max(CS), E)
    with cases.index_of(g) as ix:
        for C in CS:
            want = cases.assign_oracle(cases.logits(cen[:C], g))
            cases.assert_assign(ix.assign(cen[:C]), want, f"C {C}")
            assert want[0].min() >= 0 and (C == 1 or len(np.unique(want[0])) > 1 or N == 1)


def test_assign_does_not_depend_on_the_span_hook_and_covers_many_blocks():
    """The assignment cuts no spans and no row chunks (one block per 64 rows walks every centroid tile): the
    search's span hook at 64 columns changes nothing, and 4200 rows -- past the 256-row chunk of the searches
    and the 4096 of a full grid row -- are 66 blocks of one launch."""
    rng = np.random.default_rng(4200)
    g, cen = unit_rows(rng, 4200, 16), unit_rows(rng, 130, 16)
    want = cases.assign_oracle(cases.logits(cen, g))
    with cases.index_of(g) as ix:
        try:
            span_cols(64)
            cases.assert_assign(ix.assign(cen), want, "span hook 64")
        finally:
            span_cols(0)
        cases.assert_assign(ix.assign(cen), want)


def test_assign_with_scale_and_bias():
    rng = np.random.default_rng(100)
    g, cen = unit_rows(rng, 300, 80), unit_rows(rng, 65, 80)
    with cases.index_of(g) as ix:
        cases.assert_assign(ix.assign(cen, 100.0, -3.0), cases.assign_oracle(cases.logits(cen, g, 100.0, -3.0)))


def test_ties_go_to_the_lower_centroid():
    rng = np.random.default_rng(71)
    g, cen = cases.tie_case()  # copies at 3 and 70, 64 and 129: across a centroid-tile seam
    L = cases.logits(cen, g)
    want = cases.assign_oracle(L)
    assert want[0][10] == 3 and want[0][20] == 64 and not np.isin(want[0], (70, 129)).any()
    assert not np.array_equal(want[0], cases.assign_oracle(L, tie_high=True)[0])
    with cases.index_of(g) as ix:
        cases.assert_assign(ix.assign(cen), want)
        # every centroid the same: label 0 everywhere
        labels, _ = ix.assign(np.repeat(cen[:1], 130, axis=0))
        assert not labels.any()
    # a gallery of eight distinct rows repeated, against those rows and copies of them
    base, tg, _ = tied_gallery(rng, 1000, 64)
    cen = np.concatenate([base, base[::-1], base])
    with cases.index_of(tg) as ix:
        got = ix.assign(cen)
        cases.assert_assign(got, cases.assign_oracle(cases.logits(cen, tg)))
        assert got[0].max() < 16  # never the third copy


def test_zero_and_nan_centroids():
    rng = np.random.default_rng(9)
    g = unit_rows(rng, 200, 16)
    cen = np.zeros((3, 16), np.float32)
    cen[1, 0] = 1.0
    # scale -1, bias -0.0: an all-zero centroid scores fmaf(+0, -1, -0.0) = -0.0, centroid 1 scores -g[j][0]
    L = cases.logits(cen, g, -1.0, -0.0)
    assert (bits(L[0]) == 0x80000000).all() and (bits(L[2]) == 0x80000000).all()
    want = cases.assign_oracle(L)
    pos = g[:, 0] > 0
    assert pos.any() and not pos.all()
    # -0.0 ranks as 0 does, above every negative score; of the two zero centroids the lower; its -0.0 comes back
    assert (want[0][pos] == 0).all() and (want[0][~pos] == 1).all() and (bits(want[1][pos]) == 0x80000000).all()
    with cases.index_of(g) as ix:
        cases.assert_assign(ix.assign(cen, -1.0, -0.0), want)
        cen[2] = np.nan  # a NaN centroid never wins while a finite one exists
        L = cases.logits(cen, g, -1.0, -0.0)
        assert np.isnan(L[2]).all()
        cases.assert_assign(ix.assign(cen, -1.0, -0.0), want)
        cases.assert_assign(ix.assign(cen[::-1], -1.0, -0.0), cases.assign_oracle(L[::-1]))  # nor as centroid 0
        labels, scores = ix.assign(cen[2:3])  # alone it is everybody's nearest, with a NaN score
        assert not labels.any() and np.isnan(scores).all()


def test_masks_and_revival():
    rng = np.random.default_rng(5)
    N = 1000
    g, cen = unit_rows(rng, N, 64), unit_rows(rng, 17, 64)
    L = cases.logits(cen, g)
    dead = rng.choice(N, 150, replace=False)
    live = np.ones(N, bool)
    live[dead] = False
    allow = pattern(N)
    with cases.index_of(g) as ix:
        ix.remove(dead)
        for ok, kw in ((live, {}), (live & allow, {"allow": allow})):
            want = cases.assign_oracle(L, ok)
            got = ix.assign(cen, **kw)
            cases.assert_assign(got, want)
            assert np.array_equal(got[0] == -1, ~ok) and (bits(got[1][~ok]) == bits(NEG_INF)).all()
            assert not np.array_equal(got[0], cases.assign_oracle(L, ok, count_dead=True)[0])
        none = ix.assign(cen, allow=np.zeros(N, bool))
        assert (none[0] == -1).all() and (none[1] == NEG_INF).all()
        # a whole 64-row tile dead, and only one row of a tile allowed
        tile = (np.arange(N) // 64 != 2) & live
        one = np.arange(N) == 700
        cases.assert_assign(ix.assign(cen, allow=tile), cases.assign_oracle(L, tile))
        cases.assert_assign(ix.assign(cen, allow=one), cases.assign_oracle(L, one & live))
        new = unit_rows(rng, 2, 64)
        ix.set_rows(dead[:2], new)  # revives them
        g2, live2 = g.copy(), live.copy()
        g2[dead[:2]], live2[dead[:2]] = new, True
        got = ix.assign(cen)
        cases.assert_assign(got, cases.assign_oracle(cases.logits(cen, g2), live2))
        assert (got[0][dead[:2]] >= 0).all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_a_16_bit_gallery_assigns_as_its_rounded_rows(dt):
    rng = np.random.default_rng(16)
    g, cen = unit_rows(rng, 300, 80), unit_rows(rng, 65, 80)
    r = ROUND[dt](g)
    with cases.index_of(g, dt) as ix16, cases.index_of(r) as ix32:
        assert np.array_equal(bits(ix16.rows()), bits(r))
        got = ix16.assign(cen, 100.0, 0.0)
        cases.assert_assign(got, ix32.assign(cen, 100.0, 0.0))
        cases.assert_assign(got, cases.assign_oracle(cases.logits(cen, r, 100.0, 0.0)))
        ids = [299, 0, 7, 7]
        assert np.array_equal(bits(ix16.rows_at(ids)), bits(r[ids]))
        a, b = ix16.kmeans(init=r[:4], max_iter=3), ix32.kmeans(init=r[:4], max_iter=3)
        cases.assert_kmeans(a, b._asdict())


def test_the_device_form_writes_only_its_rows_and_is_ordered():
    import torch
    from open_clip_inference import EmbeddingIndex
    rng = np.random.default_rng(12)
    g, cen = unit_rows(rng, 1000, 64), unit_rows(rng, 65, 64)
    want = cases.assign_oracle(cases.logits(cen, g))
    guard, SL, SS = 64, -7, np.float32(-12345.0)
    with EmbeddingIndex(64, 1000) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:]).cuda()
            ix.add_device(rest.data_ptr(), 936, s1.cuda_stream)  # the assignment waits for it
        with torch.cuda.stream(s2):
            dc = torch.from_numpy(cen).cuda()
            ol = torch.full((1000 + guard,), SL, dtype=torch.int32, device="cuda")
            os_ = torch.full((1000 + guard,), float(SS), dtype=torch.float32, device="cuda")
            ix.assign_device(dc.data_ptr(), 65, ol.data_ptr(), os_.data_ptr(), 1.0, 0.0, s2.cuda_stream)
        q = unit_rows(rng, 3, 64)
        with torch.cuda.stream(s1):  # a search on another stream right after: ordered behind the assignment
            dq = torch.from_numpy(q).cuda()
            oi = torch.empty((3, 5), dtype=torch.int64, device="cuda")
            osc = torch.empty((3, 5), dtype=torch.float32, device="cuda")
            ix.search_device(dq.data_ptr(), 3, 5, oi.data_ptr(), osc.data_ptr(), 100.0, 0.0, s1.cuda_stream)
        s1.synchronize()
        s2.synchronize()
        hl, hs = ol.cpu().numpy(), os_.cpu().numpy()
        assert (hl[1000:] == SL).all() and (bits(hs[1000:]) == bits(SS)).all()
        cases.assert_assign((hl[:1000].astype(np.int64), hs[:1000]), want)
        idx, score = ix.search(q, 5, 100.0, 0.0)
        assert np.array_equal(oi.cpu().numpy(), idx) and np.array_equal(bits(osc.cpu().numpy()), bits(score))


# ---- the update -----------------------------------------------------------------------------------------
def test_integer_rows_give_the_normalised_exact_sums():
    rng = np.random.default_rng(33)
    rows = rng.integers(-8, 9, (500, 32)).astype(np.float32)
    rows[(rows == 0).all(axis=1), 0] = 1.0
    init = rows[:6].copy()
    with cases.index_of(rows) as ix:
        km = ix.kmeans(init=init, max_iter=1)
        labels = ix.assign(init)[0]
    sums = np.zeros((6, 32), np.int64)  # small integers: the true sums, exactly
    np.add.at(sums, labels, rows.astype(np.int64))
    v = sums.astype(np.float64)
    n2 = np.maximum((v * v).sum(axis=1, keepdims=True), 1.0)  # exact; 1 where a cluster is empty or cancels
    want = np.where((sums != 0).any(axis=1)[:, None], v / np.sqrt(n2), init)
    assert np.array_equal(bits(km.centroids), bits(want.astype(np.float32)))
    cases.assert_assign((km.labels, km.scores), cases.assign_oracle(cases.logits(km.centroids, rows)))
    assert np.array_equal(km.counts, cases.counts_of(km.labels, 6)) and km.moved.tolist() == [500] and km.iters == 1


def test_gaussian_rows_give_the_restated_sums_and_centroids():
    rows, init = cases.wide_rows()
    want = cases.lloyd(rows, init, 1, logits_fn=cases.logits)
    with cases.index_of(rows) as ix:
        labels = ix.assign(init)[0]
        km = ix.kmeans(init=init, max_iter=1)
        S, s = cases.kmeans_sums(ix, 4)
    assert s == cases.shift_of(rows) == 7
    assert np.array_equal(S, cases.fixed_sums(rows, labels, 4, 7))
    assert not np.array_equal(S, cases.fixed_sums(rows, labels, 4, 7, truncate=True))
    cases.assert_kmeans(km, want)
    assert np.array_equal(bits(km.centroids), bits(cases.finalise(S, cases.counts_of(labels, 4), init)))


# ---- kmeans ---------------------------------------------------------------------------------------------
def test_kmeans_recovers_the_planted_blobs_and_is_a_fixed_point():
    rows, init, blob = cases.blobs()
    want = cases.lloyd(rows, init, 25, logits_fn=cases.logits)
    with cases.index_of(rows) as ix:
        km = ix.kmeans(init=init)
        cases.assert_kmeans(km, want)
        assert np.array_equal(km.labels, blob) and km.counts.tolist() == [125] * 8 and km.moved[-1] == 0
        again = ix.kmeans(init=km.centroids)  # from a converged result: the same bits
        cases.assert_kmeans(again, dict(want, moved=np.array([1000, 0]), iters=2))
        cases.assert_assign(ix.assign(km.centroids), (km.labels, km.scores))


def test_an_unconverged_run_returns_the_labels_of_its_centroids():
    rows, init = cases.generic_rows()
    want = cases.lloyd(rows, init, 2, logits_fn=cases.logits)
    assert want["iters"] == 2 and want["moved"][-1] > 0
    with cases.index_of(rows) as ix:
        km = ix.kmeans(init=init, max_iter=2)
        cases.assert_kmeans(km, want)
        cases.assert_assign((km.labels, km.scores), ix.assign(km.centroids))
        stale = cases.lloyd(rows, init, 2, logits_fn=cases.logits, stale_labels=True)
        assert not np.array_equal(km.labels, stale["labels"])


def test_a_permuted_gallery_and_a_masked_one_give_the_same_bits():
    rows, init = cases.generic_rows()
    perm = np.random.default_rng(1).permutation(len(rows))
    ok = pattern(len(rows))
    with cases.index_of(rows) as a, cases.index_of(rows[perm]) as b, cases.index_of(rows[ok]) as c:
        ka, kb = a.kmeans(init=init, max_iter=6), b.kmeans(init=init, max_iter=6)
        assert np.array_equal(bits(ka.centroids), bits(kb.centroids))
        assert np.array_equal(ka.labels[perm], kb.labels) and np.array_equal(bits(ka.scores[perm]), bits(kb.scores))
        assert np.array_equal(ka.counts, kb.counts) and np.array_equal(ka.moved, kb.moved)
        # a filter is an index of the allowed rows alone; removed rows are too
        km, kc = a.kmeans(init=init, max_iter=6, allow=ok), c.kmeans(init=init, max_iter=6)
        cases.assert_kmeans(km, cases.lloyd(rows, init, 6, ok, logits_fn=cases.logits))
        assert np.array_equal(bits(km.centroids), bits(kc.centroids)) and np.array_equal(km.labels[ok], kc.labels)
        assert (km.labels[~ok] == -1).all() and km.moved[0] == ok.sum()
        a.remove(np.flatnonzero(~ok))
        cases.assert_kmeans(a.kmeans(init=init, max_iter=6), km._asdict())


def test_an_empty_cluster_keeps_its_centroid():
    rows, start = cases.biased_rows()
    want = cases.lloyd(rows, start, 4, logits_fn=cases.logits)
    assert want["counts"][5] == 0
    with cases.index_of(rows) as ix:
        km = ix.kmeans(init=start, max_iter=4)
    cases.assert_kmeans(km, want)
    assert km.counts[5] == 0 and np.array_equal(bits(km.centroids[5]), bits(start[5]))


def test_the_seeded_start_is_the_documented_one():
    rows, _ = cases.generic_rows()
    dead = [3, 4, 5]
    allow = np.arange(len(rows)) % 2 == 1
    with cases.index_of(rows) as ix:
        ix.remove(dead)
        ids = np.flatnonzero(ix.is_live() & allow)
        start = np.sort(np.random.default_rng(11).choice(ids, 7, replace=False))
        assert np.array_equal(bits(ix.rows_at(start)), bits(rows[start]))
        km = ix.kmeans(7, seed=11, max_iter=3, allow=allow)
        cases.assert_kmeans(km, ix.kmeans(init=rows[start], max_iter=3, allow=allow)._asdict())
        ok = allow.copy()
        ok[dead] = False
        cases.assert_kmeans(km, cases.lloyd(rows, rows[start], 3, ok, logits_fn=cases.logits))


def test_errors():
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    rows, init = cases.generic_rows()
    with EmbeddingIndex(32, 700) as ix:
        with pytest.raises(ClipError, match="Empty batch"):
            ix.assign(init)
        with pytest.raises(ClipError, match="Empty batch"):
            ix.kmeans(init=init)
        ix.add(rows)
        with pytest.raises(ValueError, match="1..65536"):
            ix.assign(np.zeros((0, 32), np.float32))
        with pytest.raises(ValueError, match="1..65536"):
            ix.assign(np.zeros((65537, 32), np.float32))
        with pytest.raises(ValueError, match="max_iter"):
            ix.kmeans(init=init, max_iter=0)
        with pytest.raises(ValueError, match="only 600 rows are live and allowed"):
            ix.kmeans(601)
        ix.remove([0])
        with pytest.raises(ValueError, match="only 599 rows"):
            ix.kmeans(600)
        for bad in ([600], [-1], [0, 1, 650]):
            with pytest.raises(ClipError, match="id out of range"):
                ix.rows_at(bad)
        assert ix.rows_at([]).shape == (0, 32)
        bad = rows[:2].copy()
        bad[0, 3], bad[1, 0] = np.inf, np.nan
        ix.set_rows([417, 20], bad)
        with pytest.raises(ClipError, match="row 20 has a non-finite element"):
            ix.kmeans(init=init)
        with pytest.raises(ClipError, match="row 417 has a non-finite element"):
            ix.kmeans(init=init, allow=np.arange(600) != 20)
        ix.remove([20, 417])  # a dead row's values do not matter
        km = ix.kmeans(init=init, max_iter=2)
        assert km.iters == 2 and (km.labels[[0, 20, 417]] == -1).all()
        # the C forms refuse what Python checks first
        from open_clip_inference import _lib
        L, lab, sc = _lib.lib(), np.empty(600, np.int64), np.empty(600, np.float32)
        cnt, mv, it = np.empty(5, np.int64), np.empty(1, np.int64), np.empty(1, np.int64)
        cen = init.copy()
        for C in (0, 65537):
            assert L.clipgpu_index_assign(ix.handle, cen.ctypes.data, C, 1.0, 0.0, None, lab.ctypes.data,
                                          sc.ctypes.data) == 1
        assert L.clipgpu_index_kmeans(ix.handle, 5, cen.ctypes.data, 0, None, lab.ctypes.data, sc.ctypes.data,
                                      cnt.ctypes.data, mv.ctypes.data, it.ctypes.data) == 1
        assert np.array_equal(bits(cen), bits(init))  # a refused call leaves the start alone


def test_clip_cluster():
    """The facade on the seeded tiny model, against kmeans of the same embeddings."""
    from open_clip_inference import Clip
    from tests.helpers import cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims = list(images())
    ims = ims + ims[:2]  # two duplicate pictures
    with clip.build_index(ims) as index:
        n = len(index)
        labels, counts, centroids = clip.cluster(index, 2, seed=5, max_iter=10)
        km = index.kmeans(2, seed=5, max_iter=10)
        assert np.array_equal(labels, km.labels) and np.array_equal(counts, km.counts)
        assert np.array_equal(bits(centroids), bits(km.centroids))
        cases.assert_kmeans(km, cases.lloyd(index.rows(), index.rows_at(np.sort(np.random.default_rng(5).choice(
            np.arange(n), 2, replace=False))), 10, logits_fn=cases.logits))
        assert counts.sum() == n and labels[0] == labels[n - 2] and labels[1] == labels[n - 1]
        allow = np.arange(n) != 0
        labels, counts, _ = clip.cluster(index, 2, seed=5, allow=allow)
        assert labels[0] == -1 and (labels[1:] >= 0).all() and counts.sum() == n - 1
