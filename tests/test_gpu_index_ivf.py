"""The embedding index's inverted lists and probed search on the GPU (EmbeddingIndex.partition, lists,
search_probed, search_probed_device, Clip.search(nprobe=); csrc/kernels/lists.hip, csrc/kernels/probe.hip), against
the oracles of tests/index_ivf_cases.py.

Every expected result is built from the library's pinned functions: the logits from similarity(queries, rows as
stored), the labels from assign(centroids), the probed lists from a search of an index that holds the centroids.
Every comparison is exact: ids with array_equal, scores on their uint32 views (index_cases.assert_same).
tests/test_cpu_index_ivf.py shows that each assertion here catches the matching mutant of its oracle."""
from contextlib import contextmanager

import numpy as np
import pytest

from tests import index_ivf_cases as cases
from tests.index_cases import ROUND, assert_same, padding, pattern, unit_rows

pytestmark = pytest.mark.gpu

E0, N0, C0, Q0, K0, P0 = 16, 300, 17, 5, 10, 2  # the defaults of the sweeps: one axis moves, the others stay


@contextmanager
def hooks(parts=0, chunk=0):
    cases.hook("clipgpu_test_probe_parts", parts)
    cases.hook("clipgpu_test_probe_chunk", chunk)
    try:
        yield
    finally:
        cases.hook("clipgpu_test_probe_parts", 0)
        cases.hook("clipgpu_test_probe_chunk", 0)


def expect(ix, stored, labels, cen, q, k, nprobe, scale=100.0, bias=0.0, allow=None):
    """The contract restated: logits_oracle over the rows that are live now, allowed and in a probed list."""
    ok = ix.is_live() if allow is None else ix.is_live() & allow
    return cases.probed_oracle(cases.logits(q, stored, scale, bias), labels, cases.library_probes(cen, q, nprobe),
                               ok, k)


def check(ix, stored, cen, q, k, nprobe, scale=100.0, bias=0.0, allow=None, labels=None, what=""):
    labels = ix.assign(cen)[0] if labels is None else labels
    want = expect(ix, stored, labels, cen, q, k, nprobe, scale, bias, allow)
    assert_same(ix.search_probed(q, k, nprobe, scale, bias, allow=allow), want, what)
    return want


# ---- shapes: one sweep per axis -------------------------------------------------------------------------
@pytest.mark.parametrize("E", [16, 80, 512])
def test_embedding_widths(E):
    """One short slab; 64 + 16; eight slabs."""
    rows, cen, label = cases.planted(E, N0, C0)
    with cases.index_of(rows) as ix:
        counts = ix.partition(cen)
        assert np.array_equal(ix.assign(cen)[0], label) and counts.tolist() == cases.lengths_for(N0, C0)
        for nprobe in (1, P0, C0):
            check(ix, rows, cen, cases.queries(E, Q0), K0, nprobe, what=f"nprobe {nprobe}")


@pytest.mark.parametrize("N", [1, 17, 300, 1200])
def test_gallery_sizes(N):
    """One row; one row more than a tile; the seams; a list of 56 tiles, which is cut into parts."""
    rows, cen, label = cases.planted(E0, N, C0)
    with cases.index_of(rows) as ix:
        assert ix.partition(cen).tolist() == cases.lengths_for(N, C0)
        for nprobe in (1, P0, C0):
            check(ix, rows, cen, cases.queries(E0, Q0), K0, nprobe, what=f"nprobe {nprobe}")


@pytest.mark.parametrize("C", [1, 3, 17, 65])
def test_list_counts_and_probe_counts(C):
    """C around the coarse search's 16- and 64-column seams; nprobe 1, 2, C and past C."""
    rows, cen, label = cases.planted(E0, N0, C)
    q = cases.queries(E0, Q0)
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        assert ix.n_lists == C
        for nprobe in sorted({1, min(2, C), C, C + 5}):
            check(ix, rows, cen, q, K0, nprobe, labels=label, what=f"nprobe {nprobe}")
            idx, score, probes = ix.search_probed(q, K0, nprobe, 100.0, 0.0, return_probes=True)
            assert probes.dtype == np.int64 and np.array_equal(probes, cases.library_probes(cen, q, nprobe))
        assert_same(ix.search_probed(q, K0, min(C + 5, 128), 100.0, 0.0), ix.search(q, K0, 100.0, 0.0))


@pytest.mark.parametrize("k", [1, 10, 16, 17, 128])
def test_result_counts(k):
    """Each list capacity of the kernel, and k above the number of probed rows: (-1, -inf) padding."""
    rows, cen, label = cases.planted(E0, N0, C0)
    q = cases.queries(E0, Q0)
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        for nprobe in (1, P0):
            want = check(ix, rows, cen, q, k, nprobe, labels=label)
            if k == 128:
                pad = want[0] == -1
                assert pad.any() and (want[1][pad] == -np.inf).all() and not pad[:, 0].all()


@pytest.mark.parametrize("Q", [1, 5, 16, 17, 260])
def test_query_counts(Q):
    """Around the coarse search's 16-row route and past one chunk of 256 rows."""
    rows, cen, label = cases.planted(E0, N0, C0)
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        check(ix, rows, cen, cases.queries(E0, Q), K0, P0, labels=label)


# ---- hooks: the seams of the launch at small sizes ------------------------------------------------------
def test_the_result_does_not_depend_on_parts_or_chunks():
    rows, cen, label = cases.planted(E0, 1200, C0)  # lists of up to 56 tiles
    q = cases.queries(E0, 17)
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        want = expect(ix, rows, label, cen, q, K0, 3)
        for parts, chunk in ((1, 0), (3, 0), (100, 0), (0, 1), (0, 7), (3, 7)):  # 100 parts: most blocks are empty
            with hooks(parts, chunk):
                assert_same(ix.search_probed(q, K0, 3, 100.0, 0.0), want, f"parts {parts} chunk {chunk}")
                assert_same(ix.search_probed(q, K0, 3, 100.0, 0.0, allow=pattern(1200)),
                            expect(ix, rows, label, cen, q, K0, 3, allow=pattern(1200)), f"masked, parts {parts}")


# ---- storage types --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_a_16_bit_index_searches_as_the_f32_index_of_its_rounded_rows(dt):
    rows, cen, _ = cases.planted(80, N0, C0)
    r = ROUND[dt](rows)
    q = cases.queries(80, Q0)
    with cases.index_of(rows, dt) as ix16, cases.index_of(r) as ix32:
        c16, c32 = ix16.partition(cen), ix32.partition(cen)
        assert np.array_equal(c16, c32)  # the labels are taken on the stored rows
        for a, b in zip(ix16.lists(), ix32.lists()):
            assert np.array_equal(a, b)
        for nprobe in (1, P0, C0):
            got = ix16.search_probed(q, K0, nprobe, 100.0, 0.0)
            assert_same(got, ix32.search_probed(q, K0, nprobe, 100.0, 0.0))
            assert_same(got, expect(ix16, r, ix16.assign(cen)[0], cen, q, K0, nprobe))
        dead = [0, 5, 299]
        ix16.remove(dead)
        assert_same(ix16.search_probed(q, K0, P0, 100.0, 0.0),
                    expect(ix16, r, ix32.assign(cen)[0], cen, q, K0, P0))


# ---- row order ------------------------------------------------------------------------------------------
def test_equal_scores_come_out_by_row_id_whatever_list_they_sit_in():
    g, cen, q, head, label = cases.tied_lists()
    L = cases.logits(q, g, 100.0, 0.0)
    same = head[:, None] == head[None, :]
    assert (L.view(np.uint32)[:, :, None] == L.view(np.uint32)[:, None, :])[:, same].all()  # equal heads tie, bit for bit
    with cases.index_of(g) as ix:
        ix.partition(cen)
        assert np.array_equal(ix.assign(cen)[0], label)  # and the copies of one head sit in all five lists
        assert all(len(set(label[head == h])) == 5 for h in range(8))
        for nprobe in (2, 3, 5):
            want = check(ix, g, cen, q, 40, nprobe, labels=label)
            first = want[0][:, :6]
            assert (head[first] == head[first[:, :1]]).all() and (np.diff(first, axis=1) > 0).all()
            assert len({int(c) for c in label[first[0]]}) > 1  # the leading ties come from more than one list
        assert_same(ix.search_probed(q, 40, 5, 100.0, 0.0), ix.search(q, 40, 100.0, 0.0))
    # thirty copies of one row: all in one list, tied for every query
    rows, cen, label = cases.planted(E0, N0, C0)
    tied = rows.copy()
    tied[100:130] = rows[7]
    with cases.index_of(tied) as ix:
        ix.partition(cen)
        check(ix, tied, cen, np.concatenate([rows[7:8], cases.queries(E0, 3)]), 40, P0)


def test_a_permuted_gallery_gives_the_permuted_result():
    rows, cen, label = cases.planted(E0, N0, C0)
    q = cases.queries(E0, Q0)
    perm = np.random.default_rng(1).permutation(N0)
    with cases.index_of(rows) as a, cases.index_of(rows[perm]) as b:
        a.partition(cen)
        b.partition(cen)
        assert np.array_equal(a.assign(cen)[0][perm], b.assign(cen)[0])
        ia, sa = a.search_probed(q, K0, P0, 100.0, 0.0)
        ib, sb = b.search_probed(q, K0, P0, 100.0, 0.0)
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))  # distinct scores: the same rows, renamed
        assert np.array_equal(ia, perm[ib])


# ---- full probe, filters and removal --------------------------------------------------------------------
def test_probing_every_list_is_the_plain_search():
    rows, cen, label = cases.planted(E0, N0, C0)
    q = cases.queries(E0, 17)
    allow = pattern(N0)
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        for k in (1, 10, 128):
            assert_same(ix.search_probed(q, k, C0, 100.0, -3.0), ix.search(q, k, 100.0, -3.0))
            assert_same(ix.search_probed(q, k, C0, 100.0, -3.0, allow=allow), ix.search(q, k, 100.0, -3.0, allow=allow))


def test_each_query_equals_a_filtered_search_of_its_probed_rows():
    """End to end against the existing search: search_probed(q)[i] == search(q[i], allow = the probed rows)."""
    rows, cen, label = cases.planted(E0, N0, C0)
    q = cases.queries(E0, Q0)
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        ix.remove([3, 4, 200])
        idx, score, probes = ix.search_probed(q, K0, 3, 100.0, 0.0, return_probes=True)
        for i in range(Q0):
            mask = np.isin(label, probes[i])
            assert_same((idx[i:i + 1], score[i:i + 1]), ix.search(q[i:i + 1], K0, 100.0, 0.0, allow=mask), f"query {i}")


def test_filters_and_removal():
    rows, cen, label = cases.planted(E0, N0, C0)
    q = cases.queries(E0, Q0)
    allow = pattern(N0)
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        lists_before = ix.lists()
        check(ix, rows, cen, q, K0, P0, allow=allow, labels=label)
        first = ix.search_probed(q, 1, P0, 100.0, 0.0)[0][:, 0]
        assert (first >= 0).all()
        ix.remove(first)  # every query's best row
        assert ix.n_lists == C0  # a removal keeps the partition
        for a, b in zip(ix.lists(), lists_before):
            assert np.array_equal(a, b)  # the id stays in its list
        for kw in ({}, {"allow": allow}):
            want = check(ix, rows, cen, q, K0, P0, labels=label, **kw)
            assert not np.isin(want[0], first).any()
            got = ix.search_probed(q, K0, P0, 100.0, 0.0, **kw)
            assert not np.isin(got[0], first).any()
        # a list whose rows are all dead, and one whose rows are all disallowed
        probes = cases.library_probes(cen, q, 1)[:, 0]
        c = int(probes[0])
        members = np.flatnonzero(label == c)
        if members.size:
            off = np.ones(N0, bool)
            off[members] = False
            check(ix, rows, cen, q, K0, P0, allow=off, labels=label)
            ix.remove(members)
            want = check(ix, rows, cen, q, K0, P0, labels=label)
            assert not np.isin(want[0], members).any()
            assert_same(ix.search_probed(q[:1], K0, 1, 100.0, 0.0), check(ix, rows, cen, q[:1], K0, 1, labels=label))
        # nothing allowed at all: padding, no error
        assert_same(ix.search_probed(q, K0, P0, 100.0, 0.0, allow=np.zeros(N0, bool)), padding(Q0, K0))


def test_a_query_whose_probed_lists_are_empty_gets_padding():
    rows, cen, label = cases.planted(E0, N0, C0)
    empty = [c for c, n in enumerate(cases.lengths_for(N0, C0)) if n == 0]
    assert len(empty) >= 2
    q = np.concatenate([cen[empty[:2]], cases.queries(E0, 2)])  # the first two queries ARE empty lists' centroids
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        idx, score, probes = ix.search_probed(q, K0, 1, 100.0, 0.0, return_probes=True)
        assert probes[:2, 0].tolist() == empty[:2]
        assert_same((idx[:2], score[:2]), padding(2, K0))
        check(ix, rows, cen, q, K0, 1, labels=label)


# ---- exports --------------------------------------------------------------------------------------------
def test_lists_counts_and_a_second_partition():
    rows, cen, label = cases.planted(E0, 1200, 65)
    with cases.index_of(rows) as ix:
        assert ix.n_lists == 0
        ix.remove([5, 6, 700])
        live = ix.is_live()
        counts = ix.partition(cen)
        labels = ix.assign(cen)[0]
        assert np.array_equal(labels[live], label[live]) and (labels[~live] == -1).all()
        want = cases.lists_oracle(labels, 65)
        got = ix.lists()
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(counts, np.bincount(labels[labels >= 0], minlength=65)) and counts.dtype == np.int64
        assert not np.isin([5, 6, 700], got[1]).any()  # a row dead at that moment is in no list
        again = ix.lists()
        assert np.array_equal(got[1], again[1])
        # other centroids replace the first partition: more than 256 lists takes the second pass of the sort
        rng = np.random.default_rng(9)
        cen2 = unit_rows(rng, 300, E0)
        counts2 = ix.partition(cen2)
        labels2 = ix.assign(cen2)[0]
        assert ix.n_lists == 300 and counts2.sum() == 1197
        want2 = cases.lists_oracle(labels2, 300)
        got2 = ix.lists()
        assert np.array_equal(got2[0], want2[0]) and np.array_equal(got2[1], want2[1])
        check(ix, rows, cen2, cases.queries(E0, Q0), K0, 8, labels=labels2)
        ix.drop_partition()
        assert ix.n_lists == 0


def test_partition_kmeans():
    rows, cen, label = cases.planted(E0, N0, C0)
    with cases.index_of(rows) as ix:
        km = ix.partition_kmeans(6, max_iter=5, seed=2)
        assert ix.n_lists == 6
        off, ids = ix.lists()
        want = cases.lists_oracle(km.labels, 6)
        assert np.array_equal(off, want[0]) and np.array_equal(ids, want[1]) and np.array_equal(np.diff(off), km.counts)
        check(ix, rows, km.centroids, cases.queries(E0, Q0), K0, 2, labels=km.labels)


# ---- stale partitions and refusals ----------------------------------------------------------------------
def test_a_mutation_makes_the_partition_stale():
    from open_clip_inference.error import ClipError
    rows, cen, label = cases.planted(E0, N0, C0)
    q = cases.queries(E0, Q0)
    with cases.index_of(rows[:280], capacity=N0) as ix:
        with pytest.raises(ClipError, match="no partition"):
            ix.search_probed(q, K0, P0)
        with pytest.raises(ClipError, match="no partition"):
            ix.lists()
        for mutate in (lambda: ix.add(rows[280:290]), lambda: ix.set_rows([3], rows[290:291]), lambda: ix.clear()):
            ix.partition(cen)
            assert ix.n_lists == C0
            ix.search_probed(q, K0, P0)
            mutate()
            assert ix.n_lists == -1
            with pytest.raises(ClipError, match="stale"):
                ix.search_probed(q, K0, P0)
            with pytest.raises(ClipError, match="stale"):
                ix.lists()
        ix.add(rows)  # after the clear
        stored = rows
        ix.partition(cen)  # again: valid
        assert ix.n_lists == C0
        check(ix, stored, cen, q, K0, P0, labels=label)
        assert_same(ix.search(q, K0, 100.0, 0.0), ix.search_probed(q, K0, C0, 100.0, 0.0))


def test_add_device_makes_the_partition_stale():
    import torch
    from open_clip_inference.error import ClipError
    rows, cen, label = cases.planted(E0, N0, C0)
    with cases.index_of(rows[:200], capacity=N0) as ix:
        ix.partition(cen)
        d = torch.from_numpy(rows[200:].copy()).cuda()
        ix.add_device(d.data_ptr(), 100, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert ix.n_lists == -1
        with pytest.raises(ClipError, match="stale"):
            ix.search_probed(cases.queries(E0, 1), K0, P0)
        ix.partition(cen)
        check(ix, rows, cen, cases.queries(E0, Q0), K0, P0, labels=label)


def test_refusals_leave_the_index_usable():
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    rows, cen, label = cases.planted(E0, N0, C0)
    q = cases.queries(E0, Q0)
    with EmbeddingIndex(E0, N0) as ix:
        with pytest.raises(ClipError, match="Empty batch"):
            ix.partition(cen)
        ix.add(rows)
        ix.partition(cen)
        for bad in (0, 129):
            with pytest.raises(ValueError, match="nprobe must be in 1..128"):
                ix.search_probed(q, K0, bad)
            with pytest.raises(ValueError, match="k must be in 1..128"):
                ix.search_probed(q, bad, P0)
        with pytest.raises(ValueError, match="1..65536"):
            ix.partition(np.zeros((0, E0), np.float32))
        with pytest.raises(ValueError, match="1..65536"):
            ix.partition(np.zeros((65537, E0), np.float32))
        with pytest.raises(ClipError, match="Shape error"):
            ix.partition(np.zeros((3, E0 + 16), np.float32))
        # the C forms refuse what Python checks first, and change nothing
        from open_clip_inference import _lib
        L, oi, os_ = _lib.lib(), np.empty((Q0, K0), np.int64), np.empty((Q0, K0), np.float32)
        for k, nprobe in ((0, 2), (129, 2), (10, 0), (10, 129)):
            assert L.clipgpu_index_search_probed(ix.handle, q.ctypes.data, Q0, k, nprobe, 100.0, 0.0, None,
                                                 oi.ctypes.data, os_.ctypes.data, None) == 1
        for C in (0, 65537):
            assert L.clipgpu_index_partition(ix.handle, cen.ctypes.data, C, None) == 1
        assert ix.n_lists == C0  # the refused calls left the partition alone
        check(ix, rows, cen, q, K0, P0, labels=label)
        assert_same(ix.search(q, K0, 100.0, 0.0), ix.search_probed(q, K0, C0, 100.0, 0.0))


# ---- the device form ------------------------------------------------------------------------------------
def test_the_device_form_is_ordered_and_takes_a_device_filter():
    import torch
    from open_clip_inference.index import pack_allow
    rows, cen, label = cases.planted(E0, N0, C0)
    q = cases.queries(E0, 17)
    allow = pattern(N0)
    guard = 8
    with cases.index_of(rows) as ix:
        ix.partition(cen)
        ix.remove([0, 9, 150])  # then a search, then the probed search on a side stream
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            dq = torch.from_numpy(q.copy()).cuda()
            oi1 = torch.empty((17, K0), dtype=torch.int64, device="cuda")
            os1 = torch.empty((17, K0), dtype=torch.float32, device="cuda")
            ix.search_device(dq.data_ptr(), 17, K0, oi1.data_ptr(), os1.data_ptr(), 100.0, 0.0, s1.cuda_stream)
        s1.synchronize()  # dq is ready for the other stream
        with torch.cuda.stream(s2):
            da = torch.from_numpy(pack_allow(allow).view(np.int32)).cuda()
            oi = torch.full((17 + guard, K0), -7, dtype=torch.int64, device="cuda")
            os_ = torch.full((17 + guard, K0), -12345.0, dtype=torch.float32, device="cuda")
            op = torch.full((17 + guard, 3), -7, dtype=torch.int64, device="cuda")
            ix.search_probed_device(dq.data_ptr(), 17, K0, 3, oi.data_ptr(), os_.data_ptr(), 100.0, 0.0,
                                    s2.cuda_stream, da.data_ptr(), op.data_ptr())
        s2.synchronize()
        want = expect(ix, rows, label, cen, q, K0, 3, allow=allow)
        hi, hs, hp = oi.cpu().numpy(), os_.cpu().numpy(), op.cpu().numpy()
        assert_same((hi[:17], hs[:17]), want)
        assert (hi[17:] == -7).all() and (hs[17:] == np.float32(-12345.0)).all() and (hp[17:] == -7).all()
        assert np.array_equal(hp[:17], cases.library_probes(cen, q, 3))
        assert_same((oi1.cpu().numpy(), os1.cpu().numpy()), ix.search(q, K0, 100.0, 0.0))
        assert_same(ix.search_probed(q, K0, 3, 100.0, 0.0, allow=allow), want)


def test_clip_search_with_nprobe():
    """The facade on the seeded tiny model: nprobe=None is today's path, nprobe=n_lists the same result."""
    from open_clip_inference import Clip
    from tests.helpers import cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims = list(images())
    texts = ["a photo of a cat", "a dog"]
    with clip.build_index(ims) as index:
        index.partition(index.rows()[:2])
        plain = clip.search(index, texts, 3)
        assert plain == clip.search(index, texts, 3, nprobe=None) and clip.search(index, texts, 3, nprobe=2) == plain
        scale, bias = clip._scale_bias()
        idx, score = index.search_probed(clip.text.embed_texts(texts), 3, 1, float(scale), float(bias))
        want = [[(int(i), float(v)) for i, v in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]
        assert clip.search(index, texts, 3, nprobe=1) == want and all(want)
