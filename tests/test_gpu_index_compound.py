"""Compound queries (EmbeddingIndex.search_compound, search_compound_device, Clip.search_all / search_any;
csrc/kernels/compound.hip) against a few lines of numpy over the full logits matrix of the terms: exact, indices
by array_equal and scores on their uint32 views.  Shapes are the smallest that reach the path named beside them."""
import numpy as np
import pytest

from tests.index_cases import ROUND, assert_same, logits_oracle, pattern, span_cols, special_rows, tied_gallery, unit_rows
from tests.index_range_cases import index_of, logits

pytestmark = pytest.mark.gpu

OPS = ("min", "max")
NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def canonical(F):
    """A zero as +0.0, a NaN as 0x7fc00000."""
    F = F + np.float32(0.0)
    F[np.isnan(F)] = NAN
    return F


def fused(L, lims, op):
    """[Q][N] from the terms' logits L [T][N]: min with a NaN if any term is one, max ignoring NaNs."""
    with np.errstate(invalid="ignore"):
        rows = [np.where(np.isnan(L[a:b]).any(0), NAN, L[a:b].min(0)) if op == "min" else np.fmax.reduce(L[a:b], 0)
                for a, b in zip(lims[:-1], lims[1:])]
    return canonical(np.stack(rows).astype(np.float32))


def lims_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def check(ix, terms, lims, L, ok, k, **kw):
    for op in OPS:
        assert_same(ix.search_compound(terms, lims, k, op, 100.0, 0.0, **kw), logits_oracle(fused(L, lims, op), ok, k), op)


@pytest.mark.parametrize("sizes,N,E,k,cols", [
    ([2], 200, 16, 10, 0),                              # the smallest
    ([1, 2, 3, 4, 5, 8, 9, 16], 1000, 80, 128, 0),      # padded groups at width 16, ragged last slab, the cap of k
    ([1, 2, 3, 4, 5, 8, 9, 16], 1000, 80, 128, 64),     # ... and one 64-column tile per span, through the merge
    ([3] * 70, 4097, 512, 16, 0),                       # several query tiles at width 4, several slabs, N past a tile
    ([2, 16], 100, 64, 128, 0),                         # k > N: (-1, -inf) padding
    ([1] * 17, 300, 64, 10, 0),                         # every width as the launch's own: 1,
    ([2] * 9, 300, 64, 10, 0),                          # 2,
    ([4] * 5, 300, 64, 10, 0),                          # 4,
    ([8] * 3, 300, 64, 10, 0),                          # 8
    ([16] * 2, 300, 64, 10, 0),                         # and 16
])
def test_shapes(sizes, N, E, k, cols):
    rng = np.random.default_rng(len(sizes) * 1000 + k)
    lims = lims_of(sizes)
    g, terms = unit_rows(rng, N, E), unit_rows(rng, int(lims[-1]), E)
    span_cols(cols)
    try:
        with index_of(g) as ix:
            check(ix, terms, lims, logits(terms, g), np.ones(N, bool), k)
    finally:
        span_cols(0)


def test_tied_scores():
    """Eight distinct rows repeated: hundreds of rows share each fused score and come out by ascending row."""
    rng = np.random.default_rng(11)
    base, g, _ = tied_gallery(rng, 3000, 64)
    terms = base[[0, 1, 2, 3, 4, 5, 6, 7, 0, 3, 6, 1, 2, 5, 7]]
    lims = lims_of([2, 3, 1, 9])
    with index_of(g) as ix:
        check(ix, terms, lims, logits(terms, g), np.ones(3000, bool), 128)
        idx, _ = ix.search_compound(terms, lims, 128, "max")
        assert (np.diff(idx[2]) > 0).all()  # one term, its own row's copies first: one score, ascending rows


def test_special_values():
    """Scores of +-0, +-inf, NaN and subnormals: the NaN rule of each op, the canonical zero, and a one-term group
    against the search itself."""
    g = special_rows()
    N, E = g.shape
    rng = np.random.default_rng(12)
    zero = np.zeros((1, E), np.float32)
    terms = np.concatenate([unit_rows(rng, 3, E), zero, -unit_rows(rng, 1, E), g[:4], zero, g[5:7]])
    lims = lims_of([1, 2, 2, 4, 1, 2, 1])  # (u) (u u) (0 -u) (g0..g3) (0) (g5 g6) -- and g6 alone, below
    terms = np.concatenate([terms, g[6:7]])
    L = logits(terms, g)
    assert np.isnan(L).any() and (L == 0).any()
    with index_of(g) as ix:
        check(ix, terms, lims, L, np.ones(N, bool), N)
        for op in OPS:
            for q in (0, 4, 6):  # the one-term groups
                got = ix.search_compound(terms[lims[q]:lims[q + 1]], [0, 1], N, op, 100.0)
                want = ix.search(terms[lims[q]:lims[q + 1]], N, 100.0)
                assert_same(got, (want[0], canonical(want[1])), (op, q))


@pytest.mark.parametrize("k", [50, 128])  # fewer, and more, than the rows that stay allowed
def test_filter_and_removal(k):
    rng = np.random.default_rng(8)
    N, lims = 300, lims_of([1, 2, 5, 16])
    g, terms = unit_rows(rng, N, 64), unit_rows(rng, 24, 64)
    allow, dead = pattern(N), rng.choice(N, 50, replace=False)
    ok = allow.copy()
    ok[dead] = False
    assert 50 < ok.sum() < 128
    with index_of(g) as ix:
        ix.remove(dead)
        check(ix, terms, lims, logits(terms, g), ok, k, allow=allow)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_storage_types(dt):
    rng = np.random.default_rng(9)
    lims = lims_of([1, 2, 3, 8, 16])
    g, terms = unit_rows(rng, 1000, 64), unit_rows(rng, 30, 64)
    with index_of(g, dt) as ix:
        check(ix, terms, lims, logits(terms, ROUND[dt](g)), np.ones(1000, bool), 40)


def test_device_form_follows_an_add_on_another_stream():
    import torch
    from open_clip_inference import EmbeddingIndex
    rng = np.random.default_rng(10)
    sizes = [3, 1, 4, 2, 4]
    lims, Q, k = lims_of(sizes), len(sizes), 20
    g, terms = unit_rows(rng, 1000, 64), unit_rows(rng, sum(sizes), 64)
    with EmbeddingIndex(64, 1000) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:]).cuda()
            ix.add_device(rest.data_ptr(), 936, s1.cuda_stream)
        for op, width in (("min", 4), ("max", 16)):  # the tight bound and the one that is always valid
            with torch.cuda.stream(s2):
                dt = torch.from_numpy(terms).cuda()
                dl = torch.from_numpy(lims.astype(np.int32)).cuda()
                di = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
                ds = torch.zeros((Q, k), dtype=torch.float32, device="cuda")
                ix.search_compound_device(dt.data_ptr(), len(terms), dl.data_ptr(), Q, k, op, di.data_ptr(), ds.data_ptr(),
                                          100.0, 0.0, s2.cuda_stream, max_terms=width)
                s2.synchronize()
            host = ix.search_compound(terms, lims, k, op, 100.0)
            assert_same((di.cpu().numpy(), ds.cpu().numpy()), host, op)
            assert_same(host, logits_oracle(fused(logits(terms, g), lims, op), np.ones(1000, bool), k), op)


def test_errors():
    from open_clip_inference import COMPOUND_TERMS_MAX, EmbeddingIndex, _lib
    assert COMPOUND_TERMS_MAX == 16
    t = np.zeros((17, 16), np.float32)
    out = np.zeros(4096, np.int64)
    L = _lib.lib()

    def raw(T, lims, k=1, op=0):
        l = np.asarray(lims, np.int64)
        rc = L.clipgpu_index_search_compound(ix.handle, t.ctypes.data, T, l.ctypes.data, len(l) - 1, k, op, 1.0, 0.0, None,
                                             out.ctypes.data, out.ctypes.data)
        return rc, L.clipgpu_last_error()

    with EmbeddingIndex(16, 8) as ix:
        with pytest.raises(Exception, match="Empty batch"):
            ix.search_compound(t[:2], [0, 2], 1, "min")
        ix.add(t[:4])
        for T, lims, what in ((2, [0, 0, 2], r"1\.\.16"), (17, [0, 17], r"1\.\.16"), (3, [0, 2, 1, 3], "ascend"),
                              (2, [1, 2], "0"), (3, [0, 2], "3")):
            with pytest.raises(ValueError, match=what):
                ix.search_compound(t[:T], lims, 1, "min")
        for k in (0, 129):
            with pytest.raises(ValueError, match=r"1\.\.128"):
                ix.search_compound(t[:2], [0, 2], k, "min")
        with pytest.raises(ValueError, match="op"):
            ix.search_compound(t[:2], [0, 2], 1, "sum")
        with pytest.raises(Exception, match="Shape error"):
            ix.search_compound(np.zeros((2, 32), np.float32), [0, 2], 1, "min")
        # the library's own refusals, through the raw call: return code 1 and a message that names the limit
        for args, msg in (((2, [0, 0, 2]), b"1..16 terms"), ((17, [0, 17]), b"1..16 terms"), ((3, [0, 2, 1, 3]), b"ascending"),
                          ((2, [1, 2]), b"start at 0"), ((3, [0, 2]), b"end at"), ((2, [0, 2], 129), b"1..128"),
                          ((2, [0, 2], 0), b"1..128"), ((2, [0, 2], 1, 2), b"CLIPGPU_COMPOUND_MIN")):
            rc, err = raw(*args)
            assert rc == 1 and msg in err, (args, err)
        assert raw(2, [0, 2])[0] == 0


def test_clip_search_all_and_any():
    """The facade on the seeded tiny model, against search_compound of the same embeddings."""
    from open_clip_inference import Clip
    from tests.helpers import TEXTS, cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    groups = [list(TEXTS[:2]), list(TEXTS[1:2]), list(TEXTS[:3])]
    flat = [t for grp in groups for t in grp]
    scale, bias = clip._scale_bias()
    with clip.build_index(images()) as index:
        for facade, op in ((clip.search_all, "min"), (clip.search_any, "max")):
            idx, score = index.search_compound(clip.text.embed_texts(flat), lims_of([2, 1, 3]), 3, op, float(scale), float(bias))
            want = [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]
            assert facade(index, groups, 3) == want and all(len(r) > 0 for r in want)
