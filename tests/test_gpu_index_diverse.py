"""Diversified search (EmbeddingIndex.search_diverse / search_diverse_device, Clip.search_diverse;
csrc/kernels/diverse.hip) against a dozen lines of numpy in float32: the pool from ix.search, G from the similarity
oracle over the pool's rows, then the greedy loop of include/clipgpu.h with the key order written as a sort on
(isnan(v), -v, t).  Exact: indices by array_equal, scores on their uint32 views.  Shapes are the smallest that
reach the path named beside them."""
import numpy as np
import pytest

from tests.index_cases import ROUND, assert_same, pattern, special_rows, tied_gallery, unit_rows
from tests.index_range_cases import index_of, logits

pytestmark = pytest.mark.gpu


def bursts(rng, Q, N, E):
    """Unit base rows, each 8 times with noise of 0.05 per element, shuffled; the queries are noisy bases too."""
    base = unit_rows(rng, -(-N // 8), E)
    noisy = lambda x: x + rng.standard_normal(x.shape).astype(np.float32) * np.float32(0.05)
    g, q = noisy(np.repeat(base, 8, 0)[:N]), noisy(base[rng.integers(0, len(base), Q)])
    g, q = (x / np.linalg.norm(x, axis=1, keepdims=True) for x in (g, q))
    return g[rng.permutation(N)], q


def oracle(ix, q, k, P, lam=0.5, scale=100.0, rows=None, **kw):
    c, l = ix.search(q, P, scale, 0.0, **kw)
    rows = ix.rows() if rows is None else rows
    lam = np.float32(lam)
    a = np.float32(1.0) - lam
    idx, score = np.full((len(q), k), -1, np.int64), np.full((len(q), k), -np.inf, np.float32)
    for i in range(len(q)):
        n = int((c[i] >= 0).sum())  # the real candidates come first
        if n == 0:
            continue
        G = logits(rows[c[i, :n]], rows[c[i, :n]], scale)
        m, taken = np.full(n, -np.inf, np.float32), [0]
        with np.errstate(invalid="ignore"):
            while len(taken) < min(k, n):
                m = np.where(G[taken[-1]] > m, G[taken[-1]], m)
                v = a * l[i, :n] - lam * m
                assert v.dtype == np.float32
                taken.append(min((t for t in range(n) if t not in taken),
                                 key=lambda t: (np.isnan(v[t]), 0.0 if np.isnan(v[t]) else -v[t], t)))
        idx[i, :len(taken)], score[i, :len(taken)] = c[i, taken], l[i, taken]
    return idx, score


@pytest.mark.parametrize("Q,N,E,k,P", [
    (1, 200, 16, 5, 16),       # the smallest: one Gram tile, E below a slab
    (5, 400, 80, 128, 128),    # full pool, every tile pair, a ragged slab; a permutation of the pool
    (3, 40, 64, 50, 64),       # N < P: padding candidates, (-1, -inf) from slot 40
    (70, 4097, 512, 10, 40),   # several query tiles in stage 1, the benchmark's E, P not a multiple of 16
    (300, 1000, 64, 8, 32),    # more than one 256-query chunk
])
def test_shapes(Q, N, E, k, P):
    g, q = bursts(np.random.default_rng(Q * 1000 + k), Q, N, E)
    with index_of(g) as ix:
        want = oracle(ix, q, k, P)
        plain = ix.search(q, k, 100.0)
        assert not np.array_equal(want[0], plain[0])  # a re-ranker that does nothing would not pass
        got = ix.search_diverse(q, k, 0.5, P, 100.0)
        assert_same(got, want)
        real = min(N, k)
        assert (got[0][:, real:] == -1).all() and np.isneginf(got[1][:, real:]).all()
        if k == P:
            assert np.array_equal(np.sort(got[0], 1), np.sort(ix.search(q, P, 100.0)[0], 1))


@pytest.mark.parametrize("lam", [0.0, 1.0, 0.3])  # the search; farthest-first; an `a` that is not exact in binary
def test_diversity(lam):
    g, q = bursts(np.random.default_rng(5), 6, 600, 64)
    with index_of(g) as ix:
        got = ix.search_diverse(q, 12, lam, 48, 100.0)
        assert_same(got, oracle(ix, q, 12, 48, lam))
        assert np.array_equal(got[0], ix.search(q, 12, 100.0)[0]) == (lam == 0.0)


def test_ties():
    """Eight distinct rows, thousands of copies, k = P = 128: every tie of v resolves by pool position."""
    base, g, _ = tied_gallery(np.random.default_rng(11), 3000, 64)
    with index_of(g) as ix:
        assert_same(ix.search_diverse(base, 128, 0.5, 128, 100.0), oracle(ix, base, 128, 128))


def test_special_values():
    """Logits of +-inf and NaN and NaN entries of G: a NaN never raises m, a NaN v ranks last, scores keep their bits."""
    s = special_rows()
    g = np.concatenate([s[:3], s[2:]])
    N, E = g.shape
    big = np.zeros((1, E), np.float32)
    big[0, 5] = 3e38  # its dot with an ordinary row overflows: logits of +inf and -inf
    q = np.concatenate([unit_rows(np.random.default_rng(12), 3, E), np.zeros((1, E), np.float32), g[6:8], big])
    with index_of(g) as ix:
        idx, score, pidx, pscore = ix.search_diverse(q, N, 0.5, N, 100.0, return_pool=True)
        assert np.isnan(pscore).any() and np.isposinf(pscore).any() and np.isneginf(pscore).any()
        assert np.isnan(logits(g, g)).any()
        assert_same((idx, score), oracle(ix, q, N, N))
        assert np.array_equal(np.sort(idx, 1), np.sort(pidx, 1))


def test_filter_and_removal():
    g, q = bursts(np.random.default_rng(8), 4, 600, 64)
    allow = pattern(600)
    with index_of(g) as ix:
        first = ix.search_diverse(q, 10, 0.5, 40, 100.0, allow=allow)
        assert_same(first, oracle(ix, q, 10, 40, allow=allow))
        assert allow[first[0]].all()
        gone = np.unique(first[0])
        ix.remove(gone)
        got = ix.search_diverse(q, 10, 0.5, 40, 100.0, allow=allow)
        assert_same(got, oracle(ix, q, 10, 40, rows=g, allow=allow))
        assert not np.isin(got[0], gone).any() and allow[got[0]].all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_storage_types(dt):
    g, q = bursts(np.random.default_rng(9), 5, 1000, 80)
    with index_of(g, dt) as ix:
        assert_same(ix.search_diverse(q, 20, 0.5, 64, 100.0), oracle(ix, q, 20, 64, rows=ROUND[dt](g)))


def test_return_pool_and_device_form_behind_an_add_on_another_stream():
    import torch
    from open_clip_inference import EmbeddingIndex
    Q, k, P = 5, 10, 40
    g, q = bursts(np.random.default_rng(10), Q, 1000, 64)
    with EmbeddingIndex(64, 1000) as ix:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ix.add(g[:64])
        with torch.cuda.stream(s1):
            rest = torch.from_numpy(g[64:]).cuda()
            ix.add_device(rest.data_ptr(), 936, s1.cuda_stream)
        with torch.cuda.stream(s2):
            dq = torch.from_numpy(q).cuda()
            di, dp = (torch.full((Q, n), -7, dtype=torch.int64, device="cuda") for n in (k, P))
            ds, dps = (torch.zeros((Q, n), dtype=torch.float32, device="cuda") for n in (k, P))
            ix.search_diverse_device(dq.data_ptr(), Q, k, di.data_ptr(), ds.data_ptr(), 0.5, P, 100.0, 0.0,
                                     s2.cuda_stream, d_pool_idx=dp.data_ptr(), d_pool_score=dps.data_ptr())
            s2.synchronize()
        want, pool = oracle(ix, q, k, P, rows=g), ix.search(q, P, 100.0)
        assert_same((di.cpu().numpy(), ds.cpu().numpy()), want)
        assert_same((dp.cpu().numpy(), dps.cpu().numpy()), pool)
        host = ix.search_diverse(q, k, 0.5, P, 100.0, return_pool=True)
        assert_same(host[:2], want)
        assert_same(host[2:], pool)


def test_errors():
    from open_clip_inference import EmbeddingIndex, _lib
    L = _lib.lib()
    t = np.zeros((4, 16), np.float32)
    out = np.zeros(4096, np.int64)

    def raw(k, pool, lam):
        rc = L.clipgpu_index_search_diverse(ix.handle, t.ctypes.data, 1, k, pool, lam, 1.0, 0.0, None, out.ctypes.data,
                                            out.ctypes.data, None, None)
        return rc, L.clipgpu_last_error()

    with EmbeddingIndex(16, 8) as ix:
        with pytest.raises(Exception, match="Empty batch"):
            ix.search_diverse(t[:1], 1)
        rc, err = raw(1, 32, 0.5)
        assert rc == 1 and b"Empty batch" in err
        ix.add(t)
        for k, pool, lam, msg in ((0, 32, 0.5, r"1\.\.128"), (129, 128, 0.5, r"1\.\.128"), (5, 4, 0.5, "k <= pool"),
                                  (5, 129, 0.5, r"1\.\.128"), (2, 8, -0.1, "diversity"), (2, 8, 1.5, "diversity"),
                                  (2, 8, float("nan"), "diversity")):
            with pytest.raises(ValueError, match=msg):
                ix.search_diverse(t[:1], k, lam, pool)
            rc, err = raw(k, pool, lam)
            assert rc == 1 and msg.replace("\\", "").encode() in err, err
        with pytest.raises(Exception, match="Shape error"):
            ix.search_diverse(np.zeros((1, 32), np.float32), 1)
        assert raw(2, 8, 0.5)[0] == 0


def test_clip_search_diverse():
    """The facade on the seeded tiny model, against index.search_diverse of the same embeddings."""
    from open_clip_inference import Clip
    from tests.helpers import TEXTS, cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    scale, bias = clip._scale_bias()
    with clip.build_index(images()) as index:
        idx, score = index.search_diverse(clip.text.embed_texts(TEXTS), 3, 0.7, 8, float(scale), float(bias))
        want = [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]
        assert clip.search_diverse(index, TEXTS, 3, 0.7, 8) == want and all(len(r) > 0 for r in want)
