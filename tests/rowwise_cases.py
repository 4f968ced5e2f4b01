"""Inputs, fp64 references and derived error bounds of the row-kernel tests (tests/test_gpu_rowwise.py),
with a numpy-f32 emulation of the kernels' arithmetic so that tests/test_cpu_rowwise_bounds.py can check
every bound on the CPU before a GPU result is held against it.

Derivation (include/clipgpu_testing.h states the same): a wave's row reduction is at most 20 per-lane
adds plus 6 shuffle levels; with the divide, subtract, multiply and fma every f32 result carries fewer
than K = 64 roundings of u = 2^-24.
  f32 LayerNorm output:  f32bound = K u (|ref| + |gamma| rstd mean|x_row| + |beta|)
      (the middle term is the error of the mean, relative to |x| and not to x - mean, scaled as the
      output scales it)
  statistics:            |mean - ref| <= K u mean|x_row|,  |rstd / ref - 1| <= K u
  16-bit LayerNorm:      1.01 rel |ref| + f32bound,  rel = 2^-8 (bf16) / 2^-11 (f16): one output rounding
  MAP attention:         1.01 rel |ref| + 1e-4 max|v|
  l2norm:                32 u |ref|
"""
import numpy as np

from oracle import clip_ref

BF16, F16 = 0, 1
U = 2.0 ** -24
K_ROUNDINGS = 64
EPS = 1e-5


def round16(x, dtype):
    """x rounded to the nearest bf16 / f16 (ties to even), as f32."""
    x = np.asarray(x, np.float32)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def rel16(dtype):
    return 2.0 ** -8 if dtype == BF16 else 2.0 ** -11


def stream(x, x16):
    """x as the residual stream stores it (f32, or rounded to f16), as f32."""
    x = np.asarray(x, np.float32)
    return x.astype(np.float16).astype(np.float32) if x16 else x


def ln_params(D, seed):
    rng = np.random.default_rng(seed)
    w = (1 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    return w, b


def stream_rows(rows, D, seed):
    """Residual-stream-like rows (as lnf_case of test_gpu_kernels): per-row scale and offset, three
    channels 40x the rest."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, D)) * rng.uniform(0.5, 4.0, (rows, 1)) + rng.standard_normal((rows, 1))
    x[:, rng.choice(D, min(3, D), replace=False)] *= 40.0
    return x.astype(np.float32)


CONSTANTS = [2.5, -0.375, 1.3330078125, 96.0]  # exact in f16 (and so in f32)


def ln_rows_input(rows, D, seed, x16):
    """Row r is of kind r % 4: 0 ordinary; 1 |mean| = 100 std (a one-pass variance loses it);
    2 three channels 40x the rest; 3 constant (rstd = 1 / sqrt(eps))."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, D)) * rng.uniform(0.5, 4.0, (rows, 1)) + rng.standard_normal((rows, 1))
    for r in range(rows):
        kind = r % 4
        if kind == 1:
            s = rng.uniform(0.5, 4.0)
            x[r] = s * rng.standard_normal(D) + 100.0 * s * (1 if r % 8 == 1 else -1)
        elif kind == 2:
            x[r, rng.choice(D, 3, replace=False)] *= 40.0
        elif kind == 3:
            x[r] = CONSTANTS[(r // 4) % len(CONSTANTS)]
    return stream(x, x16)


def ln_ref(x, w, b, eps=EPS):
    """fp64 LayerNorm of f32 inputs (eps as the kernel holds it, in f32): (ref, mean, rstd)."""
    x = np.asarray(x, np.float64)
    e = float(np.float32(eps))
    mu = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + e)
    return clip_ref.layer_norm(x, np.asarray(w, np.float64), np.asarray(b, np.float64), e), mu[..., 0], rstd[..., 0]


def f32bound(ref, x, w, b, rstd):
    mabs = np.abs(np.asarray(x, np.float64)).mean(-1, keepdims=True)
    return K_ROUNDINGS * U * (np.abs(ref) + np.abs(w) * rstd[..., None] * mabs + np.abs(b))


def bound16(dtype, ref, x, w, b, rstd):
    return 1.01 * rel16(dtype) * np.abs(ref) + f32bound(ref, x, w, b, rstd)


def check_ln32(got, x, w, b, eps=EPS):
    ref, _, rstd = ln_ref(x, w, b, eps)
    err = np.abs(got - ref)
    bound = f32bound(ref, x, w, b, rstd)
    assert np.all(err <= bound), (float((err / bound).max()), np.argwhere(err > bound)[:4].tolist())


def check_ln16(dtype, got, x, w, b, eps=EPS):
    ref, _, rstd = ln_ref(x, w, b, eps)
    err = np.abs(got - ref)
    bound = bound16(dtype, ref, x, w, b, rstd)
    assert np.all(err <= bound), (float((err / bound).max()), np.argwhere(err > bound)[:4].tolist())


def check_stats(stats, x, eps=EPS):
    """stats [rows][2] = f32 (mean, rstd) of the rows of x."""
    one = np.ones(x.shape[-1])
    _, mu, rstd = ln_ref(x, one, 0 * one, eps)
    mabs = np.abs(np.asarray(x, np.float64)).mean(-1)
    merr = np.abs(stats[:, 0] - mu)
    assert np.all(merr <= K_ROUNDINGS * U * mabs), (float((merr / np.maximum(mabs, 1e-300)).max() / U),
                                                    np.argwhere(merr > K_ROUNDINGS * U * mabs)[:4].tolist())
    rerr = np.abs(stats[:, 1] / rstd - 1)
    assert np.all(rerr <= K_ROUNDINGS * U), (float(rerr.max() / U), np.argwhere(rerr > K_ROUNDINGS * U)[:4].tolist())


def ln_emulate_f32(x, w, b, eps=EPS):
    """Two-pass LayerNorm in numpy f32 (the kernels' arithmetic up to summation order):
    (out f32, stats [rows][2])."""
    x = np.asarray(x, np.float32)
    D = np.float32(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=np.float32) / D
    d = x - mean
    var = (d * d).sum(-1, keepdims=True, dtype=np.float32) / D
    rstd = np.float32(1) / np.sqrt(var + np.float32(eps))
    out = d * rstd * np.asarray(w, np.float32) + np.asarray(b, np.float32)
    assert out.dtype == np.float32
    return out, np.concatenate([mean, rstd], -1)


def map_case(B, N, H, hd, dtype, span, seed):
    """q [H*hd] f32 (differs per head), kv [B*N][2*H*hd] rounded to dtype, with k scaled so that the
    scores q.k / sqrt(hd) reach +-span in every head (the largest |score| of a head is span).  At span
    60 the shifted exponents reach -120 (probabilities down to 1e-52, flushed to 0 in f32); at span 100
    exp of an unshifted score overflows f32 (exp(88.7)), so a softmax without the max subtraction fails;
    at span 3 the probabilities are spread over many keys, so the V reduction sums many terms."""
    rng = np.random.default_rng(seed)
    D = H * hd
    q = rng.standard_normal(D).astype(np.float32)
    k = rng.standard_normal((B, N, H, hd))
    s = np.einsum("bnhd,hd->bnh", k, q.reshape(H, hd).astype(np.float64)) / np.sqrt(hd)
    k *= (span / np.abs(s).max(axis=(0, 1)))[None, None, :, None]
    v = rng.standard_normal((B, N, H, hd)) * 2.0
    kv = np.concatenate([k.reshape(B * N, D), v.reshape(B * N, D)], 1)
    return q, round16(kv, dtype)


def map_ref(q, kv, B, N, H, hd):
    """fp64 softmax(q.k / sqrt(hd)) @ v per (image, head): [B][H*hd]."""
    D = H * hd
    k = kv[:, :D].astype(np.float64).reshape(B, N, H, hd)
    v = kv[:, D:].astype(np.float64).reshape(B, N, H, hd)
    s = np.einsum("bnhd,hd->bhn", k, q.astype(np.float64).reshape(H, hd)) / np.sqrt(hd)
    return np.einsum("bhn,bnhd->bhd", clip_ref.softmax(s), v).reshape(B, D)


def map_bound(dtype, ref, kv, D):
    return 1.01 * rel16(dtype) * np.abs(ref) + 1e-4 * np.abs(kv[:, D:]).max()


def map_emulate_f32(q, kv, B, N, H, hd):
    """The MAP kernel's arithmetic in numpy f32 (up to summation order and the exp's last bits)."""
    D = H * hd
    f = np.float32
    k = kv[:, :D].reshape(B, N, H, hd).astype(f)
    v = kv[:, D:].reshape(B, N, H, hd).astype(f)
    s = np.einsum("bnhd,hd->bhn", k, q.reshape(H, hd).astype(f)).astype(f) * f(1.0 / np.sqrt(f(hd)))
    e = np.exp(s - s.max(-1, keepdims=True)).astype(f)
    inv = f(1) / e.sum(-1, keepdims=True, dtype=f)
    return (np.einsum("bhn,bnhd->bhd", e, v).astype(f) * inv).reshape(B, D)


def l2_rows(B, E, seed, shift=0):
    """Row r is of kind (r + shift) % 3: 0 random; 1 all zero; 2 of norm 1e-20."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, E)) * rng.uniform(0.1, 30.0, (B, 1))
    for r in range(B):
        kind = (r + shift) % 3
        if kind == 1:
            x[r] = 0.0
        elif kind == 2:
            x[r] *= 1e-20 / np.sqrt((x[r] ** 2).sum())
    return x.astype(np.float32)


def l2_ref(x):
    return clip_ref.l2_normalize(np.asarray(x, np.float64), float(np.float32(1e-12)))


def l2_emulate_f32(x):
    x = np.asarray(x, np.float32)
    n = np.maximum(np.sqrt((x * x).sum(-1, keepdims=True, dtype=np.float32)), np.float32(1e-12))
    return x / n
