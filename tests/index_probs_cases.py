"""Inputs, the float64 oracle and the derived error bound B of the embedding index's probability search
(EmbeddingIndex.search_probs; the PROBS kernels of csrc/kernels/topk.hip), with a numpy-f32 model of the
kernels' (m, s) accumulation and three mutants, so that tests/test_cpu_index_probs.py can check on the CPU
that B holds for correct arithmetic and rejects a column counted twice, a dropped span and an omitted
rescale.  tests/test_gpu_index_probs.py holds the kernels to the same B.  No GPU import.

What the kernels do, for one query row over the set A of counted columns (logits l, all f32):
  lane:   the 16 lanes (column % 16) that share an accumulator row each keep a running (m, s), fed in
          ascending column order: a logit above m does s = s * expf(m - l) + 1, m = l; any other does
          s += expf(l - m).  n_lane = ceil(span columns / 16) logits per lane and span at the most.
  span:   M_span = max of the 16 m (exact); each lane rescales once, s * expf(m - M_span) (by exactly 1
          where m == M_span); a four-level add tree.  One pair per (row, span).
  merge:  M = max of the spans' m (exact); lane j % 64 adds s_j * expf(m_j - M) over its spans in ascending
          order (ceil(spans / 64) terms), then a six-level add tree gives S.
  result: p = expf(l - M) / S.

Bound (first order in u = 2^-24, the unit roundoff, and ue = 2^-23, one ulp: the accuracy of expf in the
HIP math API's table of device functions), for the relative error of S and of every p, R = max (M - l)
over the finite logits of A:
  every exp is expf(fl(a - b)): the subtraction's rounding moves the argument by at most u |a - b|, the
  exponential by that much relatively, and the function adds ue.  Along the path of one logit into S the
  arguments are (m_then - l), then one (m_old - m_new) per later rescale of its lane, then (m_lane - M_span),
  then (M_span - M): they are all >= 0 and telescope to M - l <= R.  So the subtractions cost R u in all.
    the logit's own expf                                   ue
    later steps of its lane, each an add (u) or a rescale
      (expf ue, multiply u, add u; an fma: less)           (n_lane - 1) (ue + 2 u)
    the span's rescale and add tree                        ue + u + 4 u
    the merge's rescale, lane chain and add tree           ue + u + (ceil(spans / 64) - 1 + 6) u
    the subtractions                                       R u
  B_S = (1 + 2^-11) * the sum of these      (products of (1 + d_i) with sum |d_i| = x <= 2^-12 stay within
                                             x (1 + x); products that fall below 2^-126 are lost, which
                                             S >= 1 and the test's absolute 2^-126 on p absorb)
  B   = B_S + (1 + 2^-11) (R u + ue + u)    (p's own subtraction, expf and the division)
The tests evaluate B at upper bounds of its arguments that hold for every span cut: n_lane <= ceil(N / 16)
(one span) and spans <= ceil(N / 64) (one tile per span); B grows with both.  At the largest test shape
(N = 1037, scale 100 on unit rows: R <= 200) that is 4.0e-5 < 2^-12 = 2.4e-4, the cap.

The matrix path the facade test compares with (softmax_rows / softmax_cols_kernel: expf(l - m), a chain or
a strided chain plus tree of at most n + 6 adds, one division) has, by the same accounting,
  B_matrix = (1 + 2^-11) (2 (R u + ue) + (n + 6) u + u).
"""
import functools

import numpy as np

U = 2.0 ** -24
UE = 2.0 ** -23
CAP = 2.0 ** -12
TINY = 2.0 ** -126
HI = 1.0 + 2.0 ** -11


def bound_sum(n_lane, spans, R):
    merge = -(-spans // 64) - 1 + 6
    return HI * (UE + (n_lane - 1) * (UE + 2 * U) + (UE + 5 * U) + (UE + U + merge * U) + R * U)


def bound(n_lane, spans, R):
    return bound_sum(n_lane, spans, R) + HI * (R * U + UE + U)


def bound_for(N, R):
    """(B, B_S) for a gallery of N rows under any span cut."""
    n_lane, spans = -(-N // 16), -(-N // 64)
    b, bs = bound(n_lane, spans, R), bound_sum(n_lane, spans, R)
    assert bs < b <= CAP, (N, R, b)
    return b, bs


def bound_matrix(n, R):
    return HI * (2 * (R * U + UE) + (n + 6) * U + U)


def unit_rows(rng, n, E):
    x = rng.standard_normal((n, E)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def rows(N, E=64, Q=70):
    """Seeded L2-normalised Gaussian gallery [N][E] and queries [Q][E]; shared, never written to."""
    rng = np.random.default_rng(9000 + 17 * N + E)
    g, q = unit_rows(rng, N, E), unit_rows(rng, Q, E)
    g.setflags(write=False)
    q.setflags(write=False)
    return g, q


def oracle(L):
    """L: f32 logits [Q][n] of the counted rows alone.  -> (p* f64 [Q][n], M f32 [Q], S* f64 [Q], R): the
    max-subtracted softmax in float64; a NaN or +inf logit makes its row NaN, as exp(inf - inf) does."""
    L = np.asarray(L, np.float32)
    Q, n = L.shape
    if n == 0:
        return np.zeros((Q, 0)), np.full(Q, -np.inf, np.float32), np.zeros(Q), 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        M = np.fmax.reduce(L, axis=1)  # ignores NaN, as fmaxf and f32::max do
        e = np.exp(L.astype(np.float64) - M.astype(np.float64)[:, None])
        S = e.sum(axis=1)
        p = e / S[:, None]
        fin = np.isfinite(L) & np.isfinite(M)[:, None]  # a row with M = +inf is NaN throughout: no bound to hold
        R = float(np.max(np.where(fin, M[:, None].astype(np.float64) - L, 0.0))) if fin.any() else 0.0
    return p, M, S, R


def check(got, L, allow, what=""):
    """got = search_probs(..., "softmax", allow=allow, return_norm=True); L: the f32 logits matrix [Q][N] of
    every row; allow: bool [N], the live allowed rows.  Holds probabilities and (M, S) to B."""
    idx, score, prob, norm = got
    A = np.flatnonzero(allow)
    p, M, S, R = oracle(L[:, A])
    B, BS = bound_for(L.shape[1], R)  # the spans are cut over all N rows, allowed or not
    n = min(idx.shape[1], len(A))
    assert (idx[:, n:] == -1).all() and np.isneginf(score[:, n:]).all() and (prob[:, n:] == 0).all(), what
    assert prob.dtype == np.float32 and norm.dtype == np.float32
    if len(A) == 0:
        assert np.isneginf(norm[:, 0]).all() and (norm[:, 1] == 0).all(), what
        return B
    assert (idx[:, :n] >= 0).all() and allow[idx[:, :n]].all(), what
    pos = np.searchsorted(A, idx[:, :n])
    want = np.take_along_axis(p, pos, 1)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(prob[:, :n]), nan), what
    err = np.abs(prob[:, :n].astype(np.float64) - want)
    ok = nan | (err <= B * want + TINY)
    assert ok.all(), (what, float(np.nanmax(err / np.maximum(want, TINY))), B)
    assert np.array_equal(norm[:, 0].view(np.uint32), M.view(np.uint32)), what
    snan = np.isnan(S)
    assert np.array_equal(np.isnan(norm[:, 1]), snan), what
    assert (snan | (np.abs(norm[:, 1].astype(np.float64) - S) <= BS * S)).all(), what
    if n == len(A) and not nan.any():  # every row returned: the probabilities sum to one
        assert (np.abs(prob[:, :n].astype(np.float64).sum(axis=1) - 1.0) <= len(A) * B).all(), what
    return B


# ---- a numpy-f32 model of the accumulation, and its mutants ---------------------------------------------
F = np.float32


def expf(x):
    """An f32 exp within half an ulp (the kernels' expf is allowed one)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return F(np.exp(np.float64(F(x))))


def ms_add(m, s, l, rescale=True):
    if l > m:
        return l, F(F(s * (expf(F(m - l)) if rescale else F(1))) + F(1))
    if l != -np.inf:
        return m, F(s + expf(F(l - m)))
    return m, s


def tree(v, shifts, op):
    v = np.array(v, np.float32)
    for sh in shifts:
        v = op(v, np.roll(v, -sh)).astype(np.float32)
    return v[0]


def model_span(logits, mutant=None):
    """One span's pair from its logits in column order: lane = column % 16."""
    cols = list(range(len(logits)))
    if mutant == "twice":
        cols.append(len(logits) // 2)
    m, s = [F(-np.inf)] * 16, [F(0)] * 16
    for c in cols:
        m[c % 16], s[c % 16] = ms_add(m[c % 16], s[c % 16], F(logits[c]), rescale=mutant != "no rescale")
    M = tree(m, (8, 4, 2, 1), np.fmax)
    scaled = [s[i] if m[i] == M else F(s[i] * expf(F(m[i] - M))) for i in range(16)]
    return M, tree(scaled, (8, 4, 2, 1), np.add)


def model(logits, spans, mutant=None):
    """(M, S) of one query row: `spans` = the column counts of consecutive spans."""
    pairs, at = [], 0
    for i, n in enumerate(spans):
        if not (mutant == "span dropped" and i == 1):
            pairs.append(model_span(logits[at:at + n], mutant if i == 0 else None))
        at += n
    M = F(-np.inf)
    for m, _ in pairs:
        M = np.fmax(M, m)
    lanes = [F(0)] * 64
    for j, (m, s) in enumerate(pairs):
        lanes[j % 64] = F(lanes[j % 64] + (s if m == M else F(s * expf(F(m - M)))))
    return M, tree(lanes, (8, 4, 2, 1, 16, 32), np.add)


MUTANTS = ["twice", "span dropped", "no rescale"]
