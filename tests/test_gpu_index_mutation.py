"""Row removal and in-place replacement of the embedding index (EmbeddingIndex.remove / set_rows / live /
is_live) on the GPU.  A removed row is a row that no search may return: `remove` then search must equal,
bit for bit, the search with the corresponding `allow` (tests/test_gpu_index_filter.py pins that against
an index of the allowed rows only), and after `set_rows` a search equals that of a fresh index built from
the final rows.  Indices are compared with == and scores as uint32 views."""
import numpy as np
import pytest

from tests.index_cases import ROUND, assert_same, bits_equal_with_nans, logits_oracle, padding, route, search_once, \
    unit_rows

pytestmark = pytest.mark.gpu

SCALE, BIAS = 100.0, 0.0
N, E = 200, 64


@pytest.fixture(scope="module")
def gq():
    rng = np.random.default_rng(2024)
    g, q = unit_rows(rng, N, E), unit_rows(rng, 5, E)
    g.setflags(write=False)
    q.setflags(write=False)
    return g, q


def both_routes(fn):
    for r in (1, 2):
        with route(r):
            fn(f"route {r}")


def test_remove_equals_the_corresponding_allow(gq):
    from open_clip_inference import EmbeddingIndex
    g, q = gq
    dead = np.array([0, 15, 16, 63, 64, 65, 127, 199] + list(range(130, 190)))
    allow = np.ones(N, bool)
    allow[dead] = False
    with EmbeddingIndex(E, N) as filtered, EmbeddingIndex(E, N) as ix:
        filtered.add(g)
        ix.add(g)
        ix.remove(dead)
        assert len(ix) == N and ix.live == N - len(dead)
        assert np.array_equal(ix.is_live(), allow)

        def check(what):
            for k in (10, 128):
                got = ix.search(q, k, SCALE, BIAS)
                assert_same(got, filtered.search(q, k, SCALE, BIAS, allow=allow), what)
                assert not np.isin(got[0], dead).any()
        both_routes(check)
        assert filtered.live == N and filtered.is_live().all()  # the other index is untouched


def test_remove_and_allow_are_anded(gq):
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    g, q = gq
    rng = np.random.default_rng(1)
    L = similarity(q, g, SCALE, BIAS, "logits", 1)
    dead = rng.choice(N, 70, replace=False)
    allow = rng.random(N) < 0.5
    both = allow.copy()
    both[dead] = False
    assert 0 < both.sum() < allow.sum()
    with EmbeddingIndex(E, N) as ix:
        ix.add(g)
        ix.remove(dead)

        def check(what):
            assert_same(ix.search(q, 10, SCALE, BIAS, allow=allow), logits_oracle(L, both, 10), what)
            # allowing only dead rows leaves nothing
            only_dead = np.zeros(N, bool)
            only_dead[dead] = True
            assert_same(ix.search(q, 10, SCALE, BIAS, allow=only_dead), padding(len(q), 10), what)
        both_routes(check)


def test_live_counts_through_duplicates_and_repeats(gq):
    from open_clip_inference import EmbeddingIndex
    g, _ = gq
    with EmbeddingIndex(E, N) as ix:
        ix.add(g)
        assert ix.live == N and ix.is_live().all() and ix.is_live().dtype == np.bool_
        ix.remove([])  # nothing
        assert ix.live == N
        ix.remove([7, 7, 7, 31, 32])
        assert ix.live == N - 3
        ix.remove([7])  # already dead: a no-op
        ix.remove(np.array([32, 33], np.int32))
        assert ix.live == N - 4 and len(ix) == N
        want = np.ones(N, bool)
        want[[7, 31, 32, 33]] = False
        assert np.array_equal(ix.is_live(), want)


def test_a_bad_id_changes_nothing(gq):
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    g, q = gq
    with EmbeddingIndex(E, N + 10) as ix:
        ix.add(g)
        before = ix.search(q, 10, SCALE, BIAS)
        for bad in ([3, N], [3, -1], [N + 5], [1, 2, 1 << 40]):  # N .. N + 9 are inside the capacity, not the size
            with pytest.raises(ClipError, match="out of range"):
                ix.remove(bad)
            assert ix.live == N and ix.is_live().all()
            assert_same(ix.search(q, 10, SCALE, BIAS), before, f"after remove({bad})")
        ix.remove([3])
        for bad in ([4, N], [-1]):
            with pytest.raises(ClipError, match="out of range"):
                ix.set_rows(bad, g[:len(bad)])
            assert ix.live == N - 1 and not ix.is_live()[3]
        with pytest.raises(ClipError, match="out of range"):
            ix.remove([5, N])
        assert ix.live == N - 1 and ix.is_live()[5]


def test_add_after_remove_appends_live_rows(gq):
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.engine import similarity
    g, q = gq
    L = similarity(q, g, SCALE, BIAS, "logits", 1)
    with EmbeddingIndex(E, N) as ix:
        ix.add(g[:100])
        ix.remove([5, 50, 99])
        ix.add(g[100:])
        assert len(ix) == N and ix.live == N - 3
        want = np.ones(N, bool)
        want[[5, 50, 99]] = False
        assert np.array_equal(ix.is_live(), want)
        both_routes(lambda what: assert_same(ix.search(q, 128, SCALE, BIAS), logits_oracle(L, want, 128), what))


def test_clear_then_add_gives_all_rows_live(gq):
    from open_clip_inference import EmbeddingIndex
    g, q = gq
    with EmbeddingIndex(E, N) as ix:
        ix.add(g)
        ix.remove(np.arange(0, N, 2))
        assert ix.live == N // 2
        ix.clear()
        assert len(ix) == 0 and ix.live == 0 and ix.is_live().shape == (0,)
        ix.add(g[:150])
        assert ix.live == 150 and ix.is_live().all()
        assert_same(ix.search(q, 10, SCALE, BIAS), search_once(q, g[:150], 10, SCALE, BIAS))
        ix.remove([1])  # a first removal again, on the cleared bitmap
        assert ix.live == 149 and ix.is_live().sum() == 149


def test_set_rows_revives_a_slot_and_equals_a_fresh_index(gq):
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    g, q = gq
    rng = np.random.default_rng(8)
    new = unit_rows(rng, 4, E)
    ids = [64, 3, 199, 100]  # not ascending: row i of `new` goes to ids[i]
    final = g.copy()
    final[ids] = new
    with EmbeddingIndex(E, N) as ix:
        ix.add(g)
        ix.remove([3, 64, 150])
        ix.set_rows(ids, new)  # 3 and 64 come back with new rows, 199 and 100 are replaced alive, 150 stays dead
        assert ix.live == N - 1 and not ix.is_live()[150] and ix.is_live()[[3, 64]].all()
        assert np.array_equal(ix.rows().view(np.uint32), final.view(np.uint32))
        allow = np.ones(N, bool)
        allow[150] = False

        def check(what):
            with EmbeddingIndex(E, N) as fresh:
                fresh.add(final)
                assert_same(ix.search(q, 128, SCALE, BIAS), fresh.search(q, 128, SCALE, BIAS, allow=allow), what)
        both_routes(check)
        ix.set_rows([150], g[150:151])
        assert ix.live == N and ix.is_live().all()
        both_routes(lambda what: assert_same(ix.search(q, 10, SCALE, BIAS), search_once(q, final, 10, SCALE, BIAS), what))
        # duplicate ids: refused, nothing written, nothing revived
        ix.remove([9])
        before = ix.rows()
        with pytest.raises(ClipError, match="duplicate"):
            ix.set_rows([9, 20, 9], new[:3])
        assert np.array_equal(ix.rows().view(np.uint32), before.view(np.uint32))
        assert ix.live == N - 1 and not ix.is_live()[9]
        with pytest.raises(ClipError):
            ix.set_rows([1, 2], new[:3])  # two ids for three rows


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_set_rows_rounds_as_add_does(dt):
    """The special rows of the storage-type tests (subnormals, the overflow edge, signed zeros, infinities,
    NaN) written by set_rows come back from rows() as numpy's rounding, the bits that add stores."""
    from open_clip_inference import EmbeddingIndex
    from tests.index_cases import special_rows
    x = special_rows()
    n, Ex = x.shape
    rng = np.random.default_rng(4)
    filler = unit_rows(rng, n + 3, Ex)
    ids = np.arange(n)[::-1] + 2  # reversed, shifted: rows 2 .. n + 1
    want = ROUND[dt](filler)
    want[ids] = ROUND[dt](x)
    with EmbeddingIndex(Ex, n + 3, dtype=dt) as ix, EmbeddingIndex(Ex, n, dtype=dt) as added:
        ix.add(filler)
        ix.remove(ids[:2])
        ix.set_rows(ids, x)
        added.add(x)
        bits_equal_with_nans(ix.rows(), want)
        bits_equal_with_nans(ix.rows()[ids], added.rows())
        assert ix.live == n + 3


def test_an_all_removed_index_returns_padding(gq):
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    g, q = gq
    with EmbeddingIndex(E, N) as ix:
        ix.add(g)
        ix.remove(np.arange(N))
        assert ix.live == 0 and len(ix) == N and not ix.is_live().any()
        both_routes(lambda what: assert_same(ix.search(q, 10, SCALE, BIAS), padding(len(q), 10), what))
        assert_same(ix.search(q, 10, SCALE, BIAS, allow=np.ones(N, bool)), padding(len(q), 10))
        ix.clear()
        with pytest.raises(ClipError, match="Empty batch"):
            ix.search(q, 3)
