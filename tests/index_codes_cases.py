"""Oracles of the embedding index's int8 codes and coded search (EmbeddingIndex.enable_codes, codes, search_coded;
csrc/kernels/codes.hip), the inputs the GPU tests use, and mutants of each oracle that those tests' assertions
must catch (tests/test_cpu_index_codes.py runs both on the CPU).

  codes_oracle       a row's int8 codes and f32 scale: the rule of include/clipgpu.h in numpy f32 operations.
  coarse_oracle      the coarse scores [Q][N]: the int dot product of the codes times the row's scale.
  candidates_oracle  per query the `refine` best allowed rows by (coarse, then lower row): the search's order.
  coded_oracle       per query, index_cases.logits_oracle over its candidates: the contract of search_coded.

On the GPU the logits come from `similarity`, the library's pinned function, so the re-rank is tested against
the existing search's oracle and the coarse stage against integers.  The library is imported inside the
functions that need it, so this module imports without a GPU."""
import functools

import numpy as np

from tests.index_cases import logits_oracle, padding, unit_rows
from tests.index_ivf_cases import hook, index_of, logits, logits64, queries  # noqa: F401  (shared with the IVF suite)

F127 = np.float32(127)


# ---- oracles and their mutants --------------------------------------------------------------------------
def codes_oracle(rows, half_away=False, top=127):
    """(codes int8 [n][E], scale f32 [n]).  Mutants: half_away rounds x.5 away from zero instead of to even;
    top=128 maps the row maximum to 128 (inv = 128 / m) and cuts at int8's 127 -- with inv = 127 / m a wider clamp
    alone changes nothing, |x_i * inv| <= 127 (1 + 2^-23) rounds to at most 127."""
    x = np.ascontiguousarray(rows, np.float32)
    with np.errstate(all="ignore"):
        m = np.abs(x).max(axis=1)  # a NaN propagates through np.max
        inv = np.float32(top) / m
        zero = ~np.isfinite(m) | (m == 0) | ~np.isfinite(inv)
        p = x * np.where(zero, np.float32(0), inv)[:, None]
        assert p.dtype == np.float32
        r = np.trunc(p + np.copysign(np.float32(0.5), p)) if half_away else np.rint(p)
        scale = m / F127
    codes = np.clip(np.where(zero[:, None], 0, r), -127, 127).astype(np.int8)
    return codes, np.where(zero, np.float32(0), scale).astype(np.float32)


def coarse_oracle(cq, cg, sg, neg=False, no_scale=False, no_flip=False):
    """f32 [Q][N]: f32(int dot) * scale[j], negated when the logit scale is negative.  Mutants: the scale left
    out; the sign flip left out."""
    d = cq.astype(np.int64) @ cg.astype(np.int64).T
    assert np.abs(d).max(initial=0) < 1 << 24
    c = d.astype(np.float32)
    if not no_scale:
        c = c * sg[None, :].astype(np.float32)
    return -c if (neg and not no_flip) else c


def candidates_oracle(coarse, ok, refine, tie_high=False, count_dead=False):
    """(cand int64 [Q][refine], coarse f32 [Q][refine]), -1 / -inf padded: the search's order on the coarse scores.
    Mutants: tie_high gives equal scores to the HIGHER row (the order they are met in, walked backwards);
    count_dead ignores ok."""
    N = coarse.shape[1]
    ok = np.ones(N, bool) if count_dead else ok
    if tie_high:
        idx, sc = logits_oracle(coarse[:, ::-1], ok[::-1], refine)
        return np.where(idx >= 0, N - 1 - idx, -1), sc
    return logits_oracle(coarse, ok, refine)


def coded_oracle(L, cand, k):
    """(idx int64 [Q][k], score f32 [Q][k]) from the full logits: per query the plain search over its candidates."""
    Q, N = L.shape
    out_i, out_s = padding(Q, k)
    for q in range(Q):
        mask = np.zeros(N, bool)
        mask[cand[q][cand[q] >= 0]] = True
        out_i[q], out_s[q] = (a[0] for a in logits_oracle(L[q:q + 1], mask, k))
    return out_i, out_s


def expect(L, stored, q, ok, k, refine, neg=False, **mutant):
    """(result, candidates, coarse) of a coded search of `stored` rows, from the logits L [Q][N]."""
    cg, sg = codes_oracle(stored)
    cq, _ = codes_oracle(q)
    cand, cs = candidates_oracle(coarse_oracle(cq, cg, sg, neg), ok, refine, **mutant)
    return coded_oracle(L, cand, k), cand, cs


def list_layout(cand):
    """What the re-rank reads: (ids int32 [Q][refine], offsets int32 [2 Q + 1], lists int64 [Q]); list 2q = the
    candidates of query q, list 2q + 1 = its padding."""
    Q, R = cand.shape
    valid = (cand >= 0).sum(axis=1)
    off = np.empty(2 * Q + 1, np.int32)
    off[0::2] = np.arange(Q + 1) * R
    off[1::2] = np.arange(Q) * R + valid
    return np.where(cand >= 0, cand, 0).astype(np.int32), off, 2 * np.arange(Q, dtype=np.int64)


# ---- inputs, computed once and never written to ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gallery(E, N, seed=0):
    """Unit rows times a per-row factor in [0.5, 2): distinct, asymmetric, and with different scales."""
    rng = np.random.default_rng(7001 * E + N + 31 * seed)
    g = unit_rows(rng, N, E) * rng.uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    g = np.ascontiguousarray(g, np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def special_rows(E):
    """Rows that hold every case of the coding rule, then ordinary rows with different maxima."""
    rng = np.random.default_rng(E)
    rows = np.zeros((12, E), np.float32)
    rows[1, :] = -0.0
    rows[2, :8] = [127, 0.5, 1.5, 2.5, -2.5, 126.5, -126.5, -3.5]  # inv == 1: halves go to even
    rows[3, :8] = [-127, 0.5, -0.5, 63.5, 64.5, -64.5, 1, -1]
    rows[4] = rng.standard_normal(E)
    rows[4, 3] = np.nan
    rows[5] = rng.standard_normal(E)
    rows[5, E - 1] = np.inf
    rows[6] = rng.standard_normal(E)
    rows[6, 0] = -np.inf
    rows[7, :3] = [1e-40, -5e-41, 0]  # 127 / m overflows
    rows[8, :4] = [3e38, -1e38, 1.5e38, 1e30]
    rows[9] = rng.standard_normal(E) * 1e-3
    rows[10] = rng.standard_normal(E) * 1e3
    rows[11, E - 1] = -0.25  # the maximum in the last element, negative
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def planted_gap(E, N, Q, k, noise=0.02):
    """(rows [N][E], queries [Q][E], gap, bound): random unit rows with k near-copies of every query planted at
    random places (unit(query + noise / sqrt(E) * Gaussian)).  Asserted here in f64: for every query the gap
    between its k-th and (k + 1)-th cosine exceeds 2 B, where B bounds |sq * sg[j] * d - q . g_j| for codes that
    are off by at most half a step: B = max(eq |g| + |q| eg + eq eg), eq = sq sqrt(E) / 2, eg = sg sqrt(E) / 2,
    plus 2^-23 relative for the one f32 multiply.  So the k best by coarse score ARE the k best rows."""
    rng = np.random.default_rng(1000003 * E + 101 * N + 7 * Q + k)
    rows, q = unit_rows(rng, N, E), unit_rows(rng, Q, E)
    where = rng.permutation(N)[:Q * k].reshape(Q, k)
    for i in range(Q):
        x = q[i] + np.float32(noise / np.sqrt(E)) * rng.standard_normal((k, E)).astype(np.float32)
        rows[where[i]] = x / np.linalg.norm(x, axis=1, keepdims=True)
    rows, q = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(q, np.float32)
    cos = np.sort(q.astype(np.float64) @ rows.astype(np.float64).T, axis=1)[:, ::-1]
    gap = float((cos[:, k - 1] - cos[:, k]).min())
    sg, sq = codes_oracle(rows)[1].astype(np.float64), codes_oracle(q)[1].astype(np.float64)
    eg, eq = sg * np.sqrt(E) / 2, sq * np.sqrt(E) / 2
    ng, nq = np.linalg.norm(rows.astype(np.float64), axis=1), np.linalg.norm(q.astype(np.float64), axis=1)
    B = float((eq[:, None] * ng[None, :] + nq[:, None] * eg[None, :] + eq[:, None] * eg[None, :]).max())
    B += 2.0**-23 * (1 + B)
    assert gap > 2 * B, f"the gap {gap} does not exceed 2 B = {2 * B}"
    for a in (rows, q):
        a.setflags(write=False)
    return rows, q, gap, B
