"""Helpers of the range search's and the self-join's tests (tests/test_cpu_index_range.py,
tests/test_gpu_index_range.py): the oracle from a full logits matrix and the exact comparisons.  No tolerance
anywhere: indices are compared with array_equal, scores on their uint32 views.

The library is imported inside the functions that need it, so this module imports without a GPU."""
import numpy as np


def range_oracle(L, thr, ok=None):
    """From the full logits matrix L [Q][N]: per query the columns where ok & (L >= thr) -- an f32 comparison,
    so a NaN never passes -- in stable descending order of the logit (ties by ascending column).  ok: bool
    [N], live AND allowed (None: every column).  Returns (lims int64 [Q + 1], idx int64, scores f32)."""
    L = np.asarray(L, np.float32)
    ok = np.ones(L.shape[1], bool) if ok is None else np.asarray(ok, bool)
    with np.errstate(invalid="ignore"):
        hit = (L >= np.float32(thr)) & ok[None, :]
    lims, idx, score = [0], [], []
    for row, h in zip(L, hit):
        cols = np.flatnonzero(h)
        cols = cols[np.argsort(-row[cols], kind="stable")]
        idx.append(cols)
        score.append(row[cols])
        lims.append(lims[-1] + len(cols))
    return (np.asarray(lims, np.int64), np.concatenate(idx).astype(np.int64),
            np.concatenate(score).astype(np.float32))


def join_oracle(S, thr, ok=None):
    """From S = similarity(g, g) [N][N]: the pairs i < j with ok[i] & ok[j] & (S[i][j] >= thr), sorted by
    (i, j).  Returns (pairs int64 [n, 2], scores f32 [n])."""
    S = np.asarray(S, np.float32)
    ok = np.ones(len(S), bool) if ok is None else np.asarray(ok, bool)
    with np.errstate(invalid="ignore"):
        hit = np.triu(S >= np.float32(thr), 1) & ok[:, None] & ok[None, :]
    i, j = np.nonzero(hit)  # row-major: (i, j) ascending
    return np.stack([i, j], axis=1).astype(np.int64), S[i, j].astype(np.float32)


def logits(q, g, scale=100.0, bias=0.0):
    from open_clip_inference.engine import similarity
    return similarity(q, g, scale, bias, "logits", 1)


def assert_range(got, want, what=""):
    lims, idx, score = got
    assert lims.dtype == np.int64 and idx.dtype == np.int64 and score.dtype == np.float32, what
    assert np.array_equal(lims, want[0]), what
    assert np.array_equal(idx, want[1]), what
    assert np.array_equal(score.view(np.uint32), want[2].view(np.uint32)), what


def assert_pairs(got, want, what=""):
    pairs, score = got
    assert pairs.dtype == np.int64 and score.dtype == np.float32 and pairs.shape == (len(score), 2), what
    assert np.array_equal(pairs, want[0]), what
    assert np.array_equal(score.view(np.uint32), want[1].view(np.uint32)), what


def index_of(g, dt="f32"):
    from open_clip_inference import EmbeddingIndex
    ix = EmbeddingIndex(g.shape[1], len(g), dtype=dt)
    ix.add(g)
    return ix
