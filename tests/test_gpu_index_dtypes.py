"""A 16-bit embedding index (EmbeddingIndex(dtype="f16" / "bf16")) on the GPU.  The contract of
include/clipgpu.h: rows are rounded to nearest even on the device, and a search returns exactly what
the f32 path returns on widen(round(rows)).  So the expected result is tests/index_cases.py's
`expected` (the full logits matrix, stably sorted) on the numpy-rounded gallery, and every comparison
is == on indices and on uint32 views of scores."""
import ctypes

import numpy as np
import pytest

from tests.index_cases import ROUND, assert_same, bits_equal_with_nans, expected, route, routes_for, search16, \
    span_cols, special_rows, tied_gallery, unit_rows

pytestmark = pytest.mark.gpu

CODES = {"f32": 0, "f16": 1, "bf16": 2}


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_rows_are_rounded_as_the_header_says(dt):
    """add and add_device store round-to-nearest-even rows (subnormals, the overflow edge, signed zeros,
    infinities, NaN): rows() gives back numpy's rounding of the CPU file's special rows, bit for bit."""
    import torch
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    x = special_rows()
    want = ROUND[dt](x)
    n, E = x.shape
    with EmbeddingIndex(E, n, dtype=dt) as a, EmbeddingIndex(E, n + 3, dtype=dt) as b:
        a.add(x)
        d = torch.from_numpy(x).cuda()
        b.add_device(d.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        assert len(a) == len(b) == n
        bits_equal_with_nans(a.rows(), want)
        bits_equal_with_nans(b.rows(), want)
        bits_equal_with_nans(a.rows(3, 5), want[3:8])  # a sub-range
        bits_equal_with_nans(b.rows(n - 1), want[n - 1:])
        for first, cnt in ((-1, 2), (0, 0), (0, n + 1), (n, 1), (3, n - 2)):
            with pytest.raises(ClipError):
                a.rows(first, cnt)


def test_an_f32_index_returns_its_rows_unchanged():
    from open_clip_inference import EmbeddingIndex
    x = special_rows()
    with EmbeddingIndex(x.shape[1], len(x)) as ix:
        ix.add(x)
        bits_equal_with_nans(ix.rows(), x)
        bits_equal_with_nans(ix.rows(2, 3), x[2:5])


SHAPES = [(1, 1, 16, 1), (3, 64, 64, 64), (1, 5, 64, 10), (16, 129, 48, 7), (17, 1000, 80, 20), (70, 4097, 512, 10),
          (2, 300, 768, 128)]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("Q,N,E,k", SHAPES)
def test_search_is_exact_on_the_rounded_rows(Q, N, E, k, dt):
    rng = np.random.default_rng(1000 * Q + N)
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    gr = ROUND[dt](g)
    for scale, bias in ((100.0, 0.0), (10.0, -10.0)):
        want = expected(q, gr, k, scale, bias)
        for r in routes_for(Q):
            with route(r):
                assert_same(search16(q, g, k, dt, scale, bias), want, f"route {r} scale {scale}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_search_is_exact_with_many_spans(dt):
    rng = np.random.default_rng(77)
    q, g = unit_rows(rng, 17, 80), unit_rows(rng, 1000, 80)
    want = expected(q, ROUND[dt](g), 20, 100.0, 0.0)
    try:
        span_cols(64)
        assert_same(search16(q, g, 20, dt), want, "17 queries: one wide launch")
        for r in (1, 2):
            with route(r):
                assert_same(search16(q[:5], g, 20, dt), (want[0][:5], want[1][:5]), f"5 queries, route {r}")
    finally:
        span_cols(0)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_the_rounding_is_real(dt):
    """A build that quietly stored f32 would pass every comparison against itself: the 16-bit scores
    must differ from the F32 index's in nearly every entry (the rounded rows differ from the f32 rows in
    nearly every element, checked on the host first)."""
    from tests.index_cases import search_once
    Q, N, E, k = 70, 4097, 512, 10
    rng = np.random.default_rng(1000 * Q + N)
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    assert (ROUND[dt](g).view(np.uint32) != g.view(np.uint32)).mean() >= 0.95
    s32 = search_once(q, g, k)[1]
    s16 = search16(q, g, k, dt)[1]
    assert (s16.view(np.uint32) != s32.view(np.uint32)).mean() >= 0.95


def test_ties_survive_rounding():
    """The tied gallery of test_ties_come_out_by_ascending_index in f16: equal rows round to equal rows,
    so the runs of equal scores are still there and still come out by ascending index."""
    rng = np.random.default_rng(15)
    base, g, _ = tied_gallery(rng, 1000)
    q = base[:3] + np.float32(0.25) * unit_rows(rng, 3, 64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    want = expected(q, ROUND["f16"](g), 128, 100.0, 0.0)
    for r in range(3):
        same = want[1][r][1:] == want[1][r][:-1]
        assert same.sum() >= 100 and (np.diff(want[0][r])[same] > 0).all()
    for cols in (64, 0):
        try:
            span_cols(cols)
            for r in (1, 2):
                with route(r):
                    assert_same(search16(q, g, 128, "f16"), want, f"span_cols {cols} route {r}")
        finally:
            span_cols(0)


def test_handle_semantics_of_a_16_bit_index():
    from open_clip_inference import EmbeddingIndex, _lib
    from open_clip_inference.error import ClipError
    rng = np.random.default_rng(6)
    g, q = unit_rows(rng, 100, 64), unit_rows(rng, 4, 64)
    L = _lib.lib()
    assert L.clipgpu_index_dtype(None) == -1
    for dt in ("f32", "f16", "bf16"):
        with EmbeddingIndex(64, 100, dtype=dt) as ix:
            assert ix.dtype == dt and L.clipgpu_index_dtype(ix.handle) == CODES[dt]
    with EmbeddingIndex(64, 8) as ix:  # the default, and the old entry point
        assert ix.dtype == "f32" and L.clipgpu_index_dtype(ix.handle) == 0
    h = ctypes.c_void_p()
    _lib.check(L.clipgpu_index_create(0, 64, 8, ctypes.byref(h)))
    assert L.clipgpu_index_dtype(h) == 0
    L.clipgpu_index_destroy(h)
    with EmbeddingIndex(64, 100, dtype="bf16") as ix:
        gr = ROUND["bf16"](g)
        ix.add(g[:60])
        with pytest.raises(ClipError, match="index full"):
            ix.add(g[:41])
        assert len(ix) == 60  # refused: nothing added
        ix.add(g[60:])
        assert len(ix) == 100
        assert_same(ix.search(q, 12, 100.0), expected(q, gr, 12, 100.0, 0.0), "two adds")
        ix.clear()
        assert len(ix) == 0
        with pytest.raises(ClipError):
            ix.rows()
        ix.add(g[30:50])
        assert np.array_equal(ix.rows().view(np.uint32), gr[30:50].view(np.uint32))
        assert_same(ix.search(q, 12, 100.0), expected(q, gr[30:50], 12, 100.0, 0.0), "after clear")


def test_clip_build_index_f16():
    from open_clip_inference import Clip
    from tests.helpers import make_model_dir
    from tests.helpers import TEXTS, cfg_with_tokenizer, images
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims = images()
    with clip.build_index(ims, dtype="f16") as index:
        assert index.dtype == "f16" and len(index) == len(ims)
        res = clip.search(index, TEXTS[:2], k=3)
    scale, bias = clip._scale_bias()
    emb = ROUND["f16"](clip.vision.embed_images(ims))
    want = expected(clip.text.embed_texts(TEXTS[:2]), emb, 3, float(scale), float(bias))
    assert [[i for i, _ in row] for row in res] == want[0].tolist()
    got = np.array([[s for _, s in row] for row in res], np.float32)
    assert np.array_equal(got.view(np.uint32), want[1].view(np.uint32))
