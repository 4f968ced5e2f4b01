"""The device-resident embedding index (clipgpu_index_*, open_clip_inference.EmbeddingIndex) on
the GPU.  The expected result is always built from the existing full-matrix path:

    L      = similarity(q, g, scale, bias, "logits")
    idx    = np.argsort(-L, axis=1, kind="stable")[:, :k]     descending, ties by ascending index
    scores = np.take_along_axis(L, idx, 1)

Indices are compared exactly and scores as uint32 views: there is no tolerance anywhere."""
import numpy as np
import pytest

from tests.index_cases import assert_same, expected, search_once, span_cols, tied_gallery, unit_rows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Q,N,E,k", [(1, 1, 16, 1), (3, 64, 64, 64), (65, 129, 512, 10), (7, 5000, 1024, 100),
                                     (256, 4097, 512, 1), (2, 300, 768, 128), (1, 5, 64, 10)])
def test_search_matches_the_sorted_logits(Q, N, E, k):
    rng = np.random.default_rng(1000 * Q + N)
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    got = search_once(q, g, k)
    assert_same(got, expected(q, g, k, 100.0, 0.0))
    if N < k:  # (1, 5, 64, 10): five results, then five (-1, -inf)
        assert (got[0][:, N:] == -1).all() and np.isneginf(got[1][:, N:]).all()
        assert (got[0][:, :N] >= 0).all()


@pytest.mark.parametrize("E", [48, 80, 144])
def test_embedding_dims_that_end_in_a_short_slab(E):
    """The kernel stages k in slabs of 64: E = 48 is one short slab, 80 and 144 end in a 16-wide one."""
    rng = np.random.default_rng(E)
    q, g = unit_rows(rng, 5, E), unit_rows(rng, 200, E)
    assert_same(search_once(q, g, 7), expected(q, g, 7, 100.0, 0.0))


@pytest.mark.parametrize("cols,N", [(64, 1000), (128, 129)])
def test_many_spans_give_the_same_result(cols, N):
    """A forced span width: 16 spans with a ragged last one (1000 = 15 * 64 + 40), and two spans the
    second of which holds one row; the merge then does real work."""
    rng = np.random.default_rng(N)
    q, g = unit_rows(rng, 70, 128), unit_rows(rng, N, 128)
    want = expected(q, g, 20, 100.0, 0.0)
    assert_same(search_once(q, g, 20), want, "default spans")
    try:
        span_cols(cols)
        assert_same(search_once(q, g, 20), want, f"span_cols {cols}")
    finally:
        span_cols(0)


@pytest.mark.parametrize("scale,bias", [(100.0, 0.0), (-1.0, 0.0), (10.0, -10.0)])
@pytest.mark.parametrize("cols", [64, 0])
def test_ties_come_out_by_ascending_index(cols, scale, bias):
    """A gallery drawn from 8 distinct vectors: every score group is 100 - 140 exact ties that
    straddle tiles and spans (for some queries the best group is smaller than k, for some larger).
    Scale -1 inverts the order of the groups; (10, -10) is the SigLIP-style pair."""
    rng = np.random.default_rng(15)
    base, g, d = tied_gallery(rng, 1000)
    q = base[:3] + np.float32(0.25) * unit_rows(rng, 3, 64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    # the inputs do what is intended: the groups' scores are well apart (f64), so each group is real
    qd = q.astype(np.float64) @ base.astype(np.float64).T
    for row in qd:
        gaps = np.abs(row[:, None] - row[None, :])[~np.eye(8, dtype=bool)]
        assert gaps.min() > 1e-3
    assert (np.abs(d[~np.eye(8, dtype=bool)]) < 1 - 1e-3).all()  # the 8 vectors are distinct
    want = expected(q, g, 128, scale, bias)
    for r in range(3):  # ascending indices within every run of equal scores
        same = want[1][r][1:] == want[1][r][:-1]
        assert same.sum() >= 100 and (np.diff(want[0][r])[same] > 0).all()
    try:
        span_cols(cols)
        assert_same(search_once(q, g, 128, scale, bias), want)
    finally:
        span_cols(0)


def test_handle_semantics():
    import torch
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    rng = np.random.default_rng(5)
    g, q = unit_rows(rng, 264, 64), unit_rows(rng, 9, 64)
    want = expected(q, g, 12, 100.0, 0.0)
    with EmbeddingIndex(64, 264) as one, EmbeddingIndex(64, 300) as ix:
        one.add(g)
        # three adds (1, 63, 200 rows), the middle one from a torch tensor on torch's current stream
        ix.add(g[:1])
        mid = torch.from_numpy(g[1:64]).cuda()
        ix.add_device(mid.data_ptr(), 63, torch.cuda.current_stream().cuda_stream)
        ix.add(g[64:])
        assert len(ix) == len(one) == 264
        assert_same(ix.search(q, 12, 100.0), want, "three adds")
        assert_same(one.search(q, 12, 100.0), want, "one add")
        # search_device into torch tensors on a non-default stream == the host form
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dq = torch.from_numpy(q).cuda()
            di = torch.empty((9, 12), dtype=torch.int64, device="cuda")
            ds = torch.empty((9, 12), dtype=torch.float32, device="cuda")
            ix.search_device(dq.data_ptr(), 9, 12, di.data_ptr(), ds.data_ptr(), 100.0, 0.0, s.cuda_stream)
            s.synchronize()
        assert_same((di.cpu().numpy(), ds.cpu().numpy()), want, "search_device")
        # beyond the capacity: refused, nothing added
        with pytest.raises(ClipError, match="index full"):
            ix.add(g[:37])
        assert len(ix) == 264
        ix.add(g[:36])
        assert len(ix) == 300
        # k out of range
        for k in (0, 129):
            with pytest.raises(ClipError, match="k must be in 1..128"):
                ix.search(q, k)
        # clear: indices restart from 0; the other index is untouched
        ix.clear()
        assert len(ix) == 0
        with pytest.raises(ClipError, match="Empty batch"):
            ix.search(q, 3)
        ix.add(g[100:150])
        assert_same(ix.search(q, 12, 100.0), expected(q, g[100:150], 12, 100.0, 0.0), "after clear")
        assert len(one) == 264
        assert_same(one.search(q, 12, 100.0), want, "the other index")


def test_clip_build_index_and_search():
    from open_clip_inference import Clip
    from open_clip_inference.engine import similarity
    from tests.helpers import make_model_dir
    from tests.helpers import TEXTS, cfg_with_tokenizer, images
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims = images()
    with clip.build_index(ims) as index:
        assert len(index) == len(ims) and index.capacity == len(ims)
        res = clip.search(index, TEXTS[:2], k=3)
    scale, bias = clip._scale_bias()
    L = similarity(clip.text.embed_texts(TEXTS[:2]), clip.vision.embed_images(ims), float(scale), float(bias),
                   "logits", 1)
    idx = np.argsort(-L, axis=1, kind="stable")[:, :3]
    assert [[i for i, _ in row] for row in res] == idx.tolist()
    got = np.array([[s for _, s in row] for row in res], np.float32)
    assert np.array_equal(got.view(np.uint32), np.take_along_axis(L, idx, 1).view(np.uint32))
    with clip.build_index(ims, capacity=10) as index:
        assert index.capacity == 10 and len(index) == len(ims)
