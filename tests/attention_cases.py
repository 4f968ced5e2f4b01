"""Inputs, the fp64 reference and the derived per-element error bound of the self-attention kernel tests
(tests/test_gpu_attention.py), with numpy-f32 emulations of both kernels' schedules and a set of mutants,
so that tests/test_cpu_attention_bounds.py can check on the CPU that the bound holds for correct
arithmetic and rejects the mistakes it is there to catch.  No GPU import.

Layout: q / k / v are [B][N][H][HD], already rounded to the 16-bit type T; the kernels read them packed as
qkv [B*N][3*H*HD] (pack / unpack below) and write out [B*N][H*HD].

Reference (attn_ref): softmax(q k^T / sqrt(HD) + mask) v in fp64, mask = triu(-inf, 1) when causal.  With
p_ij the reference probabilities it also returns
  A[b,i,h,d] = sum_j p_ij |v_jd|
  S[b,i,h]   = max over allowed keys j of sum_d |q_id k_jd| / sqrt(HD)
  V[b,i,h,d] = sum over allowed keys j of |v_jd|.

Bound, per output element:
  bound = 1.01 (rel16(T) + 2 (HD + 8) 2^-24 S) (A + |ref|)  +  floor(T) V
  rel16 = 2^-8 (bf16) / 2^-11 (f16);  floor = 2^-25 (f16) / 0 (bf16)
Derivation.  Both kernels compute out = round_T( (sum_j round_T(e_j) v_j) / sum_j e_j ), e_j = exp2 of the
shifted base-2 score, all sums in f32.  (The sums' own roundings have no term: a lane adds at most N / 4
exponentials in sequence and the MFMA chains N / 32 steps, ~sqrt(N / 4) 2^-24 <= 1e-6 relative as the
roundings fall, against the 1.01's 5e-6 (f16) / 4e-5 (bf16) and the score term beside it.)
  rel16 A:      round_T(e_j) = e_j (1 + d_j), |d_j| <= rel16, in the numerator only (the row sum adds the
                unrounded e_j), so the numerator / denominator moves by at most rel16 sum_j p_j |v_j|.
  rel16 |ref|:  the output rounding.
  2 (HD + 8) 2^-24 S (A + |ref|):  a score is an f32 sum of HD products, then one multiply by
                scale log2 e, one subtraction (or fma) of the shift and one exp2: its error is at most
                (HD + 8) 2^-24 sum_d |q_d k_d| / sqrt(HD) in natural-log units, i.e. at most
                (HD + 8) 2^-24 S relative in e_j.  That moves the numerator by that much of A and the
                denominator by that much of 1 (of |ref| after the division).  Negligible when the
                products cancel, but with q proportional to k every product is positive and S is the
                score itself.
  floor V:      round_T(e_j) of an f16 e_j < 2^-14 is a subnormal: absolute error up to 2^-25 per key
                (spacing 2^-24), times |v_j|, summed over the allowed keys; the normaliser sum_j e_j is
                >= 1 (the maximum's e is 1).  bf16 has f32's exponent range, so no such term.
The online schedule (flash_attn_kernel) multiplies l and O by corr = exp2(m_old - m_new) per tile; corr is
one more exp2 of a difference of scores, applied to numerator and denominator alike, and is covered by the
score term.
"""
import functools

import numpy as np

from tests.rowwise_cases import BF16, F16, rel16, round16

B_SWEEP, H_SWEEP = 2, 3
LOG2E = 1.4426950408889634

# (kind, span): span is the largest allowed |score| of every (sequence, head)
KINDS = [("spread", 3), ("peaked", 60), ("peaked", 100), ("late", 60), ("late", 8), ("early", 60), ("negative", 40)]
SWEEP_KINDS = [("spread", 3), ("negative", 40)]

# whole-sequence kernel (HD 64, N <= 256): both edges of every NKT (N = 32 m, 32 m + 1) and of the wave
# count (nqt = 8 | 9 at N = 128 | 129: nqt waves, or 4 waves walking the tiles)
WHOLE_N = [1, 15, 16, 17, 32, 33, 64, 65, 77, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 255, 256]
SWEEP_N = list(range(1, 78))  # trimmed text launches every causal N up to 77
# tiled kernel: 1 to 12 key tiles (odd and even counts), a 1-key last tile, a 1-query last block, causal
# blocks whose diagonal tile is or is not the last
TILED_N64 = [257, 320, 321]
TILED_N = [1, 16, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 321, 577, 730]
TILED_CASES = [(N, 64) for N in TILED_N64] + [(N, HD) for HD in (72, 80) for N in TILED_N]


def sweep_params(cases):
    """(N, HD) -> the (N, HD, causal, dtype) both test files run, the type varying fastest."""
    return [(N, HD, causal, dtype) for N, HD in cases for causal in (0, 1) for dtype in (BF16, F16)]


def param_id(p):
    N, HD, causal, dtype = p
    return f"N{N}-hd{HD}-{'causal' if causal else 'full'}-{'bf16' if dtype == BF16 else 'f16'}"


WHOLE_PARAMS = sweep_params([(N, 64) for N in WHOLE_N])
TILED_PARAMS = sweep_params(TILED_CASES)

# The case (kind, span, N, HD, causal, dtype) of the sweep on which each mutant of emulate() must leave the
# bound (tests/test_cpu_attention_bounds.py); err / bound there, numpy on a CPU, in the comment.
MUTANT_CASES = {
    "zero_key": [("negative", 40, 65, 72, 0, F16), ("negative", 40, 77, 64, 1, BF16)],      # 785, 124
    "drop_last": [("spread", 3, 17, 64, 0, BF16), ("spread", 3, 730, 80, 0, BF16)],         # 103, 5.4
    "scale8": [("spread", 3, 65, 80, 0, BF16), ("spread", 3, 577, 72, 0, BF16)],            # 27, 3.3
    "causal_ge": [("spread", 3, 77, 64, 1, BF16), ("spread", 3, 321, 80, 1, F16)],          # 384, 7204
    "no_l_rescale": [("late", 60, 129, 72, 0, BF16), ("spread", 3, 257, 64, 0, BF16)],      # 105, 84
    "p_bf16": [("spread", 3, 17, 64, 0, F16), ("spread", 3, 65, 72, 1, F16)],               # 2.6, 2.9
}


def floor16(dtype):
    return 2.0 ** -25 if dtype == F16 else 0.0


def is_tiled(N, HD):
    """launch_attention's choice: the whole-sequence kernel takes HD 64 up to 256 keys."""
    return not (HD == 64 and N <= 256)


def pack(q, k, v):
    """q / k / v [B][N][H][HD] -> qkv [B*N][3*H*HD] f32."""
    B, N, H, HD = q.shape
    return np.ascontiguousarray(np.concatenate([x.reshape(B * N, H * HD) for x in (q, k, v)], 1), np.float32)


def unpack(qkv, B, N, H, HD):
    """qkv [B*N][3*H*HD] -> q, k, v [B][N][H][HD]."""
    x = np.asarray(qkv).reshape(B, N, 3, H, HD)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


def unpack_out(out, B, N, H, HD):
    return np.asarray(out).reshape(B, N, H, HD)


def allowed_keys(N, causal):
    """[query][key] bool: the keys the softmax of a query runs over."""
    return ~np.triu(np.ones((N, N), bool), 1) if causal else np.ones((N, N), bool)


def _bhnd(x, dt):
    return np.ascontiguousarray(np.asarray(x).transpose(0, 2, 1, 3), dt)


def attn_ref(q, k, v, causal):
    """fp64 attention of q / k / v [B][N][H][HD]: (ref, A, S, V), each [B][N][H][HD] (S [B][N][H][1])."""
    N, HD = q.shape[1], q.shape[3]
    qt, kt, vt = (_bhnd(x, np.float64) for x in (q, k, v))
    masked = ~allowed_keys(N, causal)
    p = qt @ kt.swapaxes(-1, -2)  # scores, then probabilities, in place
    p /= np.sqrt(HD)
    if causal:
        p[:, :, masked] = -np.inf
    p -= p.max(-1, keepdims=True)
    np.exp(p, out=p)
    p /= p.sum(-1, keepdims=True)
    ref, A = np.split(p @ np.concatenate([vt, np.abs(vt)], -1), 2, -1)
    sa = np.abs(qt) @ np.abs(kt).swapaxes(-1, -2)
    if causal:
        sa[:, :, masked] = 0.0
    S = sa.max(-1, keepdims=True) / np.sqrt(HD)
    V = np.cumsum(np.abs(vt), 2) if causal else np.broadcast_to(np.abs(vt).sum(2, keepdims=True), vt.shape)
    return tuple(np.ascontiguousarray(x.transpose(0, 2, 1, 3)) for x in (ref, A, S, V))


def bound(dtype, HD, ref, A, S, V):
    return 1.01 * (rel16(dtype) + 2 * (HD + 8) * 2.0 ** -24 * S) * (A + np.abs(ref)) + floor16(dtype) * V


def worst(got, ref, bnd):
    """(largest err / bound, its index) of got [B][N][H][HD]; an element with bound 0 must be exact."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bnd)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)  # a NaN output
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[i]), tuple(int(x) for x in i)


class Case:
    """One input with its reference and bound: q / k / v rounded to dtype, qkv packed."""

    def __init__(self, name, dtype, causal, q, k, v):
        self.name, self.dtype, self.causal = name, dtype, causal
        self.q, self.k, self.v = q, k, v
        self.B, self.N, self.H, self.HD = q.shape
        self.qkv = pack(q, k, v)
        self.ref, A, S, V = attn_ref(q, k, v, causal)
        self.bound = bound(dtype, self.HD, self.ref, A, S, V)

    def worst(self, out):
        """out [B*N][H*HD] (or [B][N][H][HD]) -> (err / bound, index (b, i, h, d))."""
        return worst(unpack_out(out, self.B, self.N, self.H, self.HD), self.ref, self.bound)

    def check(self, out):
        """Every element inside the bound; returns the worst err / bound."""
        r, idx = self.worst(out)
        assert r <= 1.0, f"{self.name}: err/bound = {r:.3f} at (sequence, query, head, dim) = {idx}"
        return r


@functools.lru_cache(maxsize=len(KINDS))
def raw_inputs(kind, span, B, N, H, HD, causal):
    """q, k, v [B][N][H][HD] in fp64, before the rounding to a 16-bit type (the last few are kept, read-only,
    for the other type's test).  q is scaled per (sequence, head) so that the largest allowed |score| is
    span; v = 2 randn + an offset per (sequence, head, dim), so that a wrong normaliser moves every output.
      spread:   q, k random: many keys carry weight.
      peaked:   q_i = k_pi(i) + 0.05 randn, pi(i) = (7 i + 3) mod N (mod i + 1 when causal): every query
                selects one distinct key, every product q_d k_d of that score is positive.  At span 100 an
                unshifted exp2 overflows.
      late:     k_j = 0.3 randn + 8 a_j u with a_j rising linearly in j from 0 to 1, q along the unit
                vector u: the running maximum rises in every key tile, so every tile rescales l and O.
      early:    a_j falling from 1 to 0: later tiles underflow entirely.
      negative: k_j = 0.2 randn - 4 (1 + U[0,1]) u, q along u: every score is <= about -7, so a padded
                key at score 0 would take nearly all the mass."""
    rng = np.random.default_rng([[k_ for k_, _ in KINDS].index(kind), span, B, N, H, HD, causal])
    shape = (B, N, H, HD)
    i = np.arange(N)
    if kind == "spread":
        q, k = rng.standard_normal(shape), rng.standard_normal(shape)
    elif kind == "peaked":
        k = rng.standard_normal(shape)
        pi = (7 * i + 3) % (i + 1 if causal else N)
        q = k[:, pi] + 0.05 * rng.standard_normal(shape)
    else:
        u = rng.standard_normal((B, 1, H, HD))
        u /= np.sqrt((u ** 2).sum(-1, keepdims=True))
        coef = 0.5 + rng.uniform(0, 1, (B, N, H, 1))
        q = coef * u + 0.05 * rng.standard_normal(shape)
        if kind == "negative":
            k = 0.2 * rng.standard_normal(shape) - 4 * (1 + rng.uniform(0, 1, (B, N, H, 1))) * u
        else:
            a = np.linspace(0.0, 1.0, N) if N > 1 else np.ones(1)
            if kind == "early":
                a = a[::-1]
            k = 0.3 * rng.standard_normal(shape) + 8 * a[None, :, None, None] * u
    s = _bhnd(q, np.float64) @ _bhnd(k, np.float64).swapaxes(-1, -2)
    np.abs(s, out=s)
    if causal:
        s[:, :, ~allowed_keys(N, causal)] = 0.0
    q = q * (span * np.sqrt(HD) / s.max((2, 3)))[:, None, :, None]
    v = 2 * rng.standard_normal(shape) + 3 * rng.standard_normal((B, 1, H, HD))
    for x in (q, k, v):
        x.setflags(write=False)
    return q, k, v


def make_inputs(kind, span, B, N, H, HD, causal, dtype):
    """raw_inputs rounded to dtype."""
    return tuple(round16(x, dtype) for x in raw_inputs(kind, span, B, N, H, HD, causal))


def make_case(kind, span, N, HD, causal, dtype, B=B_SWEEP, H=H_SWEEP):
    name = f"{kind}{span} N={N} HD={HD} causal={causal} {'bf16' if dtype == BF16 else 'f16'}"
    return Case(name, dtype, causal, *make_inputs(kind, span, B, N, H, HD, causal, dtype))


def packed_case(name, qkv, B, N, H, HD, causal, dtype):
    """The case of a packed qkv [B*N][3*H*HD] that is already rounded to dtype."""
    return Case(name, dtype, causal, *unpack(qkv, B, N, H, HD))


# ---------------------------------------------------------------- f32 emulations and mutants

MUTANTS = ["zero_key", "drop_last", "scale8", "causal_ge", "no_l_rescale", "p_bf16"]


def emulate(q, k, v, causal, dtype, tiled, mutant=None):
    """The kernels' arithmetic in numpy f32 (up to summation order and the exp2's last bits), out
    [B][N][H][HD] rounded to dtype.
      tiled False (attn_kernel):       whole-row base-2 softmax: s = (q.k) (log2 e / sqrt(HD)), e = exp2(s - max).
      tiled True (flash_attn_kernel):  64-key tiles with a running maximum m of the raw scores,
                                       e = exp2(fma(s, c, -m c)), corr = exp2((m_old - m_new) c) applied to l and O.
    In both P = round_T(e) before the f32 P.V, the f32 row sum adds the unrounded e, and the result is
    divided by it and rounded to T.
    Mutants (the mistakes the bound must reject):
      zero_key      one zero-padded key (score 0, v = 0) is left unmasked
      drop_last     the last key is masked as if it were padding
      scale8        scale 1/8 whatever the head dim
      causal_ge     the causal mask drops key >= query (key 0 stays)
      no_l_rescale  the online row sum is not rescaled by corr
      p_bf16        P rounded to bf16 in an f16 run"""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    B, N, H, HD = q.shape
    qt, kt, vt = (_bhnd(x, f) for x in (q, k, v))
    ok = allowed_keys(N, causal)
    if mutant == "causal_ge" and causal:
        ok = np.tril(np.ones((N, N), bool), -1)
        ok[:, 0] = True
    if mutant == "drop_last":
        ok = ok.copy()
        ok[ok.sum(1) > 1, N - 1] = False
    if mutant == "zero_key":
        kt = np.concatenate([kt, np.zeros((B, H, 1, HD), f)], 2)
        vt = np.concatenate([vt, np.zeros((B, H, 1, HD), f)], 2)
        ok = np.concatenate([ok, np.ones((N, 1), bool)], 1)
    c = f(f(LOG2E) * f(0.125)) if (mutant == "scale8" or HD == 64) else f(f(LOG2E) / np.sqrt(f(HD)))
    pdt = BF16 if mutant == "p_bf16" else dtype
    s = np.where(ok, qt @ kt.swapaxes(-1, -2), f(-np.inf))  # raw scores
    assert s.dtype == f
    with np.errstate(invalid="ignore", under="ignore"):
        if not tiled:
            s = s * c
            e = np.exp2(s - s.max(-1, keepdims=True))
            o = round16(e, pdt) @ vt
            out = o * (f(1) / e.sum(-1, keepdims=True, dtype=f))
        else:
            m = np.full((B, H, N, 1), -np.inf, f)
            l = np.zeros((B, H, N, 1), f)
            o = np.zeros((B, H, N, HD), f)
            for t in range(0, s.shape[-1], 64):
                st = s[..., t:t + 64]
                mn = np.maximum(m, st.max(-1, keepdims=True))
                corr = np.exp2((m - mn) * c)
                e = np.exp2(st * c + (-mn * c))
                l = (l if mutant == "no_l_rescale" else l * corr) + e.sum(-1, keepdims=True, dtype=f)
                o = o * corr + round16(e, pdt) @ vt[:, :, t:t + 64]
                m = mn
            out = o * (f(1) / l)
    assert out.dtype == f
    return round16(out.transpose(0, 2, 1, 3), dtype)


def emulate_case(case, mutant=None):
    return emulate(case.q, case.k, case.v, case.causal, case.dtype, is_tiled(case.N, case.HD), mutant)
