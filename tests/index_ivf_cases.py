"""Oracles of the embedding index's inverted lists and probed search (EmbeddingIndex.partition, search_probed;
csrc/kernels/lists.hip, csrc/kernels/probe.hip), the inputs the GPU tests use, and mutants of each oracle that
those tests' assertions must catch (tests/test_cpu_index_ivf.py runs both on the CPU).

  lists_oracle    the CSR of the rows by label: a stable argsort of the live labels plus a bincount cumsum.
  probes_oracle   the lists a query probes, from the logits against the centroids [Q][C]: the search's order.
  probed_oracle   per query, index_cases.logits_oracle over the rows that are allowed and whose label is probed.

On the GPU the logits come from `similarity`, the labels from `assign` and the probes from a search of an index
that holds the centroids -- the library's pinned functions -- so the probed search is tested against the
existing search and not against itself.  The library is imported inside the functions that need it, so this
module imports without a GPU."""
import functools

import numpy as np

from tests.index_cases import logits_oracle, padding, unit_rows

SEAMS = (0, 1, 15, 16, 17, 33, 65)  # list lengths: empty, shorter than a 16-row tile, around one, two and four tiles


# ---- oracles and their mutants --------------------------------------------------------------------------
def lists_oracle(labels, C, descending=False):
    """(offsets int64 [C + 1], ids int64 [n_live]).  Mutant: descending ids within a list."""
    live = np.flatnonzero(labels >= 0)
    ids = live[np.argsort(labels[live], kind="stable")].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels[live], minlength=C))]).astype(np.int64)
    if descending:
        ids = np.concatenate([ids[a:b][::-1] for a, b in zip(offsets[:-1], offsets[1:])] or [ids])
    return offsets, ids


def probes_oracle(Lc, nprobe, tie_high=False):
    """int64 [Q][nprobe]: per query the min(nprobe, C) centroids with the largest score, best first, equal scores
    to the LOWER centroid (mutant: the higher), -1 past C."""
    Q, C = Lc.shape
    if tie_high:
        idx = (C - 1 - logits_oracle(Lc[:, ::-1], np.ones(C, bool), min(nprobe, C))[0])
    else:
        idx = logits_oracle(Lc, np.ones(C, bool), min(nprobe, C))[0]
    return np.concatenate([idx, np.full((Q, nprobe - idx.shape[1]), -1, np.int64)], 1)


def probed_oracle(L, labels, probes, ok, k, by_position=False, drop_partial_tile=False, drop_last_probe=False,
                  count_dead=False):
    """(idx int64 [Q][k], score f32 [Q][k]) from the full logits L [Q][N]: per query the stable descending sort
    over the rows with ok & (label in probes[q]).  Mutants: by_position breaks equal scores by the position in the
    probed lists instead of the row id; drop_partial_tile loses the last len % 16 rows of every list;
    drop_last_probe the last probed list; count_dead ignores ok."""
    Q, N = L.shape
    ok = np.ones(N, bool) if count_dead else ok
    offsets, ids = lists_oracle(labels, int(max(labels.max(), probes.max())) + 1)
    out_i, out_s = padding(Q, k)
    for q in range(Q):
        pr = probes[q][probes[q] >= 0]
        if drop_last_probe:
            pr = pr[:-1]
        rows = []
        for c in pr:
            rows_c = ids[offsets[c]:offsets[c + 1]]
            rows.append(rows_c[:len(rows_c) // 16 * 16] if drop_partial_tile else rows_c)
        rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        rows = rows[ok[rows]]
        if not by_position:
            rows = np.sort(rows)
        order = np.argsort(-L[q, rows], kind="stable")[:k]
        out_i[q, :len(order)], out_s[q, :len(order)] = rows[order], L[q, rows[order]]
    return out_i, out_s


def brute_probed(L, labels, probes, ok, k):
    """probed_oracle restated through index_cases.logits_oracle and np.isin, as the issue words it."""
    outs = [logits_oracle(L[q:q + 1], ok & np.isin(labels, probes[q]), k) for q in range(len(L))]
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def logits(q, rows, scale=1.0, bias=0.0):
    """The GPU oracle: similarity's logits [Q][N], pinned bit for bit in tests/test_gpu_similarity.py."""
    from open_clip_inference.engine import similarity
    return similarity(np.ascontiguousarray(q, np.float32), np.ascontiguousarray(rows, np.float32), scale, bias,
                      "logits", 1)


def logits64(q, rows, scale=1.0, bias=0.0):
    """The CPU stand-in: an f64 product rounded to f32."""
    return (q.astype(np.float64) @ rows.astype(np.float64).T * scale + bias).astype(np.float32)


# ---- inputs with prescribed list lengths, computed once and never written to ----------------------------
def lengths_for(N, C):
    """C list lengths that sum to N: SEAMS cycled while rows remain, what is left over in the last list."""
    out, left = [], N
    for c in range(C):
        n = min(SEAMS[c % len(SEAMS)], left)
        out.append(n)
        left -= n
    out[-1] += left
    return out


@functools.lru_cache(maxsize=None)
def planted(E, N, C, seed=0):
    """(rows [N][E] unit f32, centroids [C][E] unit f32, label [N]): row j = unit(cen[label[j]] + 0.05 * noise), the
    labels a fixed shuffle of lengths_for(N, C).  Checked here, in f64: every row's best centroid is the
    prescribed one, with a gap above 1e-3 to the runner-up -- far above the f32 chain's rounding, so every
    correct assignment gives these lists."""
    rng = np.random.default_rng(100003 * E + 1009 * N + C + 7919 * seed)
    cen = unit_rows(rng, C, E)
    label = np.repeat(np.arange(C), lengths_for(N, C))
    label = label[rng.permutation(N)]
    x = cen[label] + np.float32(0.05) * rng.standard_normal((N, E)).astype(np.float32)
    rows = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    d = rows.astype(np.float64) @ cen.astype(np.float64).T
    assert np.array_equal(d.argmax(axis=1), label), "a row's best centroid is not the prescribed one"
    if C > 1:
        part = np.partition(d, C - 2, axis=1)
        assert (part[:, C - 1] - part[:, C - 2]).min() > 1e-3, "the gap to the runner-up is too small"
    for a in (rows, cen, label):
        a.setflags(write=False)
    return rows, cen, label


@functools.lru_cache(maxsize=None)
def queries(E, Q, seed=0):
    q = unit_rows(np.random.default_rng(31 * E + Q + 977 * seed), Q, E)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def tied_lists():
    """(rows [300][64], centroids [5][64], queries [3][64], head [300], label [300]): rows whose first 16 elements
    are one of eight heads and whose other 48 decide the list; centroids and queries are zero where the other
    side's part lies.  A query's score depends on the head alone -- the products with the zeros are exact zeros,
    added after the head's part of the k-ascending chain -- so rows with equal heads tie bit for bit, in five
    different lists."""
    rng = np.random.default_rng(64)
    heads, tails = unit_rows(rng, 8, 16), unit_rows(rng, 5, 48)
    head, label = rng.integers(0, 8, 300), np.arange(300) % 5
    noise = np.float32(0.02) * rng.standard_normal((300, 48)).astype(np.float32)
    rows = np.concatenate([heads[head], tails[label] + noise], axis=1).astype(np.float32)
    cen = np.concatenate([np.zeros((5, 16), np.float32), tails], axis=1)
    q = np.concatenate([heads[:3] + np.float32(0.1) * heads[3:6], np.zeros((3, 48), np.float32)], axis=1)
    d = rows.astype(np.float64) @ cen.astype(np.float64).T
    part = np.partition(d, 3, axis=1)
    assert np.array_equal(d.argmax(axis=1), label) and (part[:, 4] - part[:, 3]).min() > 1e-3
    for a in (rows, cen, q, head, label):
        a.setflags(write=False)
    return rows, cen, q, head, label


# ---- the library side -----------------------------------------------------------------------------------
def index_of(g, dt="f32", capacity=None):
    from open_clip_inference import EmbeddingIndex
    ix = EmbeddingIndex(g.shape[1], capacity or len(g), dtype=dt)
    ix.add(g)
    return ix


def library_probes(cen, q, nprobe):
    """The probed lists as the contract defines them: the index set a search (scale 1, bias 0) of an f32 index
    holding the centroids returns, padded with -1 to nprobe."""
    with index_of(np.ascontiguousarray(cen, np.float32)) as cx:
        idx = cx.search(q, min(nprobe, len(cen)))[0]
    return np.concatenate([idx, np.full((len(q), nprobe - idx.shape[1]), -1, np.int64)], 1)


def hook(name, value):
    from open_clip_inference import _lib
    _lib.check(getattr(_lib.lib(), name)(value))
