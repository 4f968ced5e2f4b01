"""Oracles of the embedding index's assignment and k-means (EmbeddingIndex.assign, kmeans; csrc/kernels/cluster.hip),
the inputs the GPU tests use, and mutants of each oracle that those tests' assertions must catch
(tests/test_cpu_index_cluster.py runs both on the CPU).

  assign_oracle   from a full logits matrix [C][N]: per column the largest search key (csrc/kernels/topk_key.hpp).
  shift_of, fixed_sums, finalise   the update of include/clipgpu.h restated in numpy: int64 sums of
                  llrint(ldexp(x, s)), then S / sqrt(sum S^2) in f64 with np.cumsum as the sequential sum.
  lloyd           the whole loop, with the logits from `logits_fn(centroids, rows)` [C][N].

The library is imported inside the functions that need it, so this module imports without a GPU."""
import functools

import numpy as np

from tests.index_cases import unit_rows

NEG_INF = np.float32(-np.inf)


# ---- assignment -----------------------------------------------------------------------------------------
def mono(x):
    """topk_mono of topk_key.hpp on an f32 array: u64 that orders as the floats do, NaN 0 < -inf, -0 == +0."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = np.where(b == 0x80000000, 0, b)
    m = np.where((b & 0x80000000) != 0, ~b & 0xFFFFFFFF, b | 0x80000000)
    return np.where((b & 0x7FFFFFFF) > 0x7F800000, 0, m).astype(np.uint64)


def assign_oracle(L, ok=None, tie_high=False, count_dead=False):
    """(labels int64 [N], scores f32 [N]) from L [C][N]: the centroid with the largest key (score, then the
    LOWER index); (-1, -inf) where ok is False.  Mutants: tie_high breaks ties to the higher index, count_dead
    ignores ok."""
    C, N = L.shape
    c = np.arange(C, dtype=np.uint64)[:, None]
    low = c if tie_high else (~c & np.uint64(0xFFFFFFFF))
    best = ((mono(L) << np.uint64(32)) | low).argmax(axis=0)  # keys are distinct down a column
    labels, scores = best.astype(np.int64), L[best, np.arange(N)].astype(np.float32)
    if ok is not None and not count_dead:
        labels[~ok], scores[~ok] = -1, NEG_INF
    return labels, scores


def assert_assign(got, want, what=""):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32, what
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


def logits(cen, rows, scale=1.0, bias=0.0):
    """The GPU oracle: similarity's logits [C][N], pinned bit for bit in tests/test_gpu_similarity.py."""
    from open_clip_inference.engine import similarity
    return similarity(np.ascontiguousarray(cen, np.float32), np.ascontiguousarray(rows, np.float32), scale, bias,
                      "logits", 1)


def logits64(cen, rows, scale=1.0, bias=0.0):
    """The CPU stand-in: an f64 product rounded to f32."""
    return (cen.astype(np.float64) @ rows.astype(np.float64).T * scale + bias).astype(np.float32)


# ---- the update -----------------------------------------------------------------------------------------
def shift_of(rows, ok=None, one_small=False):
    """s = 62 - e - b: e the frexp exponent of the largest |x| over the counted rows (0 if that is 0), b the bit
    length of their number.  A non-finite element raises, naming the first such row."""
    ok = np.ones(len(rows), bool) if ok is None else ok
    bad = np.flatnonzero(ok & ~np.isfinite(rows).all(axis=1))
    if bad.size:
        raise ValueError(f"row {bad[0]} has a non-finite element")
    n = int(ok.sum())
    m = float(np.abs(rows[ok]).max()) if n else 0.0
    e = int(np.frexp(m)[1]) if m else 0
    return 62 - e - n.bit_length() - (1 if one_small else 0)


def fixed_sums(rows, labels, C, s, truncate=False):
    """S int64 [C][E] = sum over labels == c of llrint(ldexp((double)x, s)), to nearest even (mutant: truncated)."""
    v = np.ldexp(rows.astype(np.float64), s)
    q = (np.trunc(v) if truncate else np.rint(v)).astype(np.int64)
    S = np.zeros((C, rows.shape[1]), np.int64)
    sel = labels >= 0
    np.add.at(S, labels[sel], q[sel])
    return S


def finalise(S, counts, prev, zero_empty=False):
    """centroid[c] = (float)(S[c] / sqrt(sum_i S[c][i]^2)) in f64, the sum sequential; a cluster with no member or
    a zero sum keeps prev[c] (mutant: becomes zeros)."""
    out = prev.copy()
    for c in range(len(S)):
        v = S[c].astype(np.float64)
        n2 = np.cumsum(v * v)[-1]
        if counts[c] > 0 and n2 > 0:
            out[c] = (v / np.sqrt(n2)).astype(np.float32)
        elif zero_empty:
            out[c] = 0
    return out


def counts_of(labels, C):
    return np.bincount(labels[labels >= 0], minlength=C).astype(np.int64)


def lloyd(rows, init, max_iter, ok=None, logits_fn=logits64, stale_labels=False, **mutant):
    """EmbeddingIndex.kmeans restated: dict(centroids, labels, scores, counts, moved, iters).  Mutants:
    stale_labels returns the labels from before the last update; tie_high / count_dead go to assign_oracle,
    one_small to shift_of, truncate to fixed_sums, zero_empty to finalise."""
    ok = np.ones(len(rows), bool) if ok is None else ok
    a_kw = {k: v for k, v in mutant.items() if k in ("tie_high", "count_dead")}
    C, cen, prev, moved = len(init), init.astype(np.float32).copy(), None, []
    s = shift_of(rows, ok, one_small=mutant.get("one_small", False))
    for t in range(1, max_iter + 1):
        labels, scores = assign_oracle(logits_fn(cen, rows), ok, **a_kw)
        moved.append(int(ok.sum()) if prev is None else int(((labels != prev) & (labels >= 0)).sum()))
        if moved[-1] == 0:
            break
        S = fixed_sums(rows, labels, C, s, truncate=mutant.get("truncate", False))
        cen = finalise(S, counts_of(labels, C), cen, zero_empty=mutant.get("zero_empty", False))
        prev = labels
        if t == max_iter and not stale_labels:
            labels, scores = assign_oracle(logits_fn(cen, rows), ok, **a_kw)
    return dict(centroids=cen, labels=labels, scores=scores, counts=counts_of(labels, C),
                moved=np.asarray(moved, np.int64), iters=len(moved))


def assert_kmeans(got, want, what=""):
    """A KMeansResult against lloyd's dict: every field, exactly."""
    assert_assign((got.labels, got.scores), (want["labels"], want["scores"]), what)
    assert got.centroids.dtype == np.float32
    assert np.array_equal(got.centroids.view(np.uint32), want["centroids"].view(np.uint32)), what
    assert np.array_equal(got.counts, want["counts"]) and got.counts.dtype == np.int64, what
    assert np.array_equal(got.moved, want["moved"]) and got.iters == want["iters"], what


# ---- inputs, computed once and never written to ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blobs():
    """(rows [1000][64], init [8][64], blob [1000]): eight well-separated planted blobs on the unit sphere, row j in
    blob j % 8, and one row of each blob as the start, so that cluster c is blob c."""
    rng = np.random.default_rng(808)
    centres = unit_rows(rng, 8, 64)
    blob = np.arange(1000) % 8
    x = centres[blob] + np.float32(0.03) * rng.standard_normal((1000, 64)).astype(np.float32)
    rows = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return rows, rows[:8].copy(), blob


@functools.lru_cache(maxsize=None)
def wide_rows():
    """(rows [1000][32], init [4][32]) whose shift is 7, so that llrint rounds: Gaussian values, one element 2^44
    (e = 45, b = 10), and in row 1 odd multiples of 2^-8 -- exact halves after the scaling, where nearest even,
    half away from zero and truncation all differ."""
    rng = np.random.default_rng(44)
    rows = rng.standard_normal((1000, 32)).astype(np.float32)
    rows[0, 0] = np.float32(2.0**44)
    rows[1] = ((2 * np.arange(32) + 1) * 2.0**-8 * np.where(np.arange(32) % 2, 1, -1)).astype(np.float32)
    init = rng.standard_normal((4, 32)).astype(np.float32)
    assert shift_of(rows) == 7
    return rows, init


@functools.lru_cache(maxsize=None)
def generic_rows():
    """(rows [600][32] unit, init [5][32]): unstructured, so two Lloyd iterations do not converge."""
    rng = np.random.default_rng(600)
    return unit_rows(rng, 600, 32), unit_rows(rng, 5, 32)


@functools.lru_cache(maxsize=None)
def tie_case():
    """(rows [500][64], centroids [130][64]): centroids 70 and 129 are copies of 3 and 64, across a centroid-tile
    seam, and each of the copied centroids is some row's nearest."""
    rng = np.random.default_rng(70)
    g, cen = unit_rows(rng, 500, 64), unit_rows(rng, 130, 64)
    cen[3], cen[64] = g[10], g[20]
    cen[70], cen[129] = cen[3], cen[64]
    return g, cen


@functools.lru_cache(maxsize=None)
def biased_rows():
    """(rows [600][32] unit, start [6][32]): rows that share a strong common component, five of them as centroids
    and a sixth centroid at minus their mean, which is nobody's nearest."""
    rng = np.random.default_rng(601)
    x = unit_rows(rng, 600, 32) + unit_rows(rng, 1, 32)
    rows = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    far = -rows.astype(np.float64).mean(axis=0)
    return rows, np.concatenate([rows[:5], (far / np.linalg.norm(far)).astype(np.float32)[None]])


def index_of(g, dt="f32", capacity=None):
    from open_clip_inference import EmbeddingIndex
    ix = EmbeddingIndex(g.shape[1], capacity or len(g), dtype=dt)
    ix.add(g)
    return ix


def kmeans_sums(ix, C):
    """(S int64 [C][E], shift) of the last update the index's kmeans ran: the library's test hook."""
    import ctypes
    from open_clip_inference import _lib
    S = np.empty((C, ix.E), np.int64)
    s = ctypes.c_int(0)
    _lib.check(_lib.lib().clipgpu_test_index_kmeans_sums(ix.handle, C, S.ctypes.data, ctypes.byref(s)))
    return S, s.value
