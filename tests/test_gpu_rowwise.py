"""Kernel-level tests of csrc/kernels/rowwise.hip and the MAP attention pool (attention.hip), each
launcher in isolation through include/clipgpu_testing.h against numpy fp64 on the inputs as the kernel
sees them (f32, or pre-rounded to the 16-bit type).

Tolerances (tests/rowwise_cases.py; tests/test_cpu_rowwise_bounds.py checks each against a numpy-f32
emulation on the CPU).  A wave's row reduction is at most 20 per-lane adds plus 6 shuffle levels; with
the divide, subtract, multiply and fma every f32 result carries fewer than 64 roundings of u = 2^-24:
  f32 LayerNorm output:  f32bound = 64 u (|ref| + |gamma| rstd mean|x_row| + |beta|)
  statistics:            |mean - ref| <= 64 u mean|x_row|,  |rstd / ref - 1| <= 64 u
  16-bit LayerNorm:      1.01 rel |ref| + f32bound, rel = 2^-8 (bf16) / 2^-11 (f16), one output rounding
  f16 stream:            the kernel normalises the row as stored; the reference takes the stored row
  MAP attention:         1.01 rel |ref| + 1e-4 max|v| (one output rounding + the absolute slack
                         test_gemm_store16_act grants f32 accumulation; the probabilities stay f32)
  l2norm:                32 u |ref|
  stem sums, gathers, casts, the stems' MX bytes (both streams), row-loop and batch independence: bit for bit.
"""
import numpy as np
import pytest

from tests import rowwise_cases as rc
from tests.rowwise_cases import BF16, F16, round16

pytestmark = pytest.mark.gpu

ERR_INVALID = 1  # CLIPGPU_ERR_INVALID
EPS = rc.EPS


def _lib():
    from open_clip_inference import _lib
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def ln_rows_rc(dtype, x16, x, w, b, mx=False):
    """clipgpu_test_ln_rows: (status, out, stats, q, qs)."""
    rows, D = x.shape
    x, w, b = _f32(x), _f32(w), _f32(b)
    out, stats = np.empty((rows, D), np.float32), np.empty((rows, 2), np.float32)
    q = np.empty((rows, D), np.uint8) if mx else None
    qs = np.empty((rows, max(D // 32, 1)), np.uint8) if mx else None
    status = _lib().lib().clipgpu_test_ln_rows(dtype, x16, rows, D, EPS, _p(x), _p(w), _p(b), _p(out), _p(stats),
                                               _p(q), _p(qs))
    return status, out, stats, q, qs


def ln_rows(dtype, x16, x, w, b, mx=False):
    status, *res = ln_rows_rc(dtype, x16, x, w, b, mx)
    _lib().check(status)
    return res


# ---------------------------------------------------------------- LayerNorm rows and statistics

LN_DIMS = [4, 128, 260, 1024, 1028, 1152, 1280]  # NV = 1 .. 5; 260 and 1028 leave one lane in the last slot


@pytest.mark.parametrize("x16", [0, 1], ids=["x32", "x16"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", LN_DIMS)
def test_ln_rows_and_stats(D, dtype, x16):
    """launch_ln_rows / launch_ln_stats on both streams at every NV and partial last slot: ordinary rows,
    |mean| = 100 std, massive channels and constant rows; 37 rows (a last block of one wave)."""
    w, b = rc.ln_params(D, D)
    x = rc.ln_rows_input(37, D, D + x16, x16)
    out, stats, _, _ = ln_rows(dtype, x16, x, w, b)
    rc.check_stats(stats, x)
    rc.check_ln16(dtype, out, x, w, b)
    const = np.arange(37) % 4 == 3  # var = 0 exactly: rstd = 1 / sqrt(eps), out = beta
    assert np.all(np.abs(stats[const, 1] * np.sqrt(np.float64(np.float32(EPS))) - 1) <= 64 * rc.U)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [260, 1152])
def test_ln_row_loop(D, dtype):
    """More rows than one resident round (launch_ln_rows / launch_ln_stats cap the grid at 8 blocks per
    CU): every wave loops, two or three rows, with the next row's loads in flight.  Checked against the
    reference, and bit for bit against 37-row launches of slices at the start, middle and end: a row's
    result must not depend on how many rows its wave loops over."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 2 * 32 * cus + 5
    w, b = rc.ln_params(D, D)
    x = np.tile(rc.ln_rows_input(1024, D, D, 0), (rows // 1024 + 1, 1))[:rows]
    x = np.ascontiguousarray(x * (1 + (np.arange(rows) % 7)[:, None]).astype(np.float32))
    out, stats, q, qs = ln_rows(dtype, 0, x, w, b, mx=(D % 32 == 0))
    rc.check_stats(stats, x)
    rc.check_ln16(dtype, out, x, w, b)
    for r0 in (0, rows // 2 - 18, rows - 37):
        o, s, q1, qs1 = ln_rows(dtype, 0, x[r0:r0 + 37], w, b, mx=(D % 32 == 0))
        assert np.array_equal(_bits(o), _bits(out[r0:r0 + 37])), r0
        assert np.array_equal(_bits(s), _bits(stats[r0:r0 + 37])), r0
        if q is not None:
            assert np.array_equal(q1, q[r0:r0 + 37]) and np.array_equal(qs1, qs[r0:r0 + 37]), r0


@pytest.mark.parametrize("x16", [0, 1], ids=["x32", "x16"])
def test_ln_refusals(x16):
    """D past 5 float4 per lane, D % 4 != 0, and an MX output with D % 32 != 0 are refused
    (CLIPGPU_ERR_INVALID) before anything is launched."""
    for D, mx in [(1284, False), (130, False), (260, True), (1028, True)]:
        x = np.ones((5, D), np.float32)
        status = ln_rows_rc(BF16, x16, x, np.ones(D), np.zeros(D), mx)[0]
        assert status == ERR_INVALID, (D, mx, status)
    w, b = rc.ln_params(256, 1)  # and the next launch is clean
    x = rc.ln_rows_input(5, 256, 1, x16)
    rc.check_ln16(BF16, ln_rows(BF16, x16, x, w, b, mx=True)[0], x, w, b)


# ---------------------------------------------------------------- stems

def layernorm_mx(x, w, b):
    L = _lib()
    rows, D = x.shape
    x = _f32(x)
    q, qs = np.empty((rows, D), np.uint8), np.empty((rows, D // 32), np.uint8)
    L.check(L.lib().clipgpu_test_layernorm_mx(rows, D, EPS, _p(x), _p(_f32(w)), _p(_f32(b)), _p(q), _p(qs)))
    return q, qs


def check_stem_outputs(run, dtype, x16, D, g1, b1, check_x):
    """The three modes of a stem hook `run(mode) -> (x_out, h, stats, q, qs)`: the stream is the same in
    every mode (check_x judges it), h = ln_1 of the stored row, mode 1's statistics are the stored row's,
    mode 2's MX bytes equal launch_ln_rows' on the stored row, on both streams (same arithmetic, same store;
    tests/test_gpu_mx_quant.py holds those bytes to the fp64 LayerNorm), and on the f32 stream
    clipgpu_test_layernorm_mx's as well."""
    x_out, h, _, _, _ = run(0)
    check_x(x_out)
    rc.check_ln16(dtype, h, x_out, g1, b1)
    x1, _, stats, _, _ = run(1)
    assert np.array_equal(_bits(x1), _bits(x_out))
    rc.check_stats(stats, x_out)
    if D % 32 == 0:
        x2, _, _, q, qs = run(2)
        assert np.array_equal(_bits(x2), _bits(x_out))
        _, _, rq, rqs = ln_rows(dtype, x16, x_out, g1, b1, mx=True)
        assert np.array_equal(q, rq) and np.array_equal(qs, rqs)
        if not x16:
            rq, rqs = layernorm_mx(x_out, g1, b1)
            assert np.array_equal(q, rq) and np.array_equal(qs, rqs)


@pytest.mark.parametrize("x16", [0, 1], ids=["x32", "x16"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,tokens,D", [(3, 5, 128), (2, 50, 768), (2, 10, 1152)])
def test_vision_stem(B, tokens, D, dtype, x16):
    """launch_vision_embed_ln: x = ln_pre(cls + pos[0]) on CLS rows (whatever the stream held there: the
    test leaves a value no other row holds), ln_pre(x) elsewhere; h = ln_1 of the row as stored."""
    L = _lib()
    rows = B * tokens
    rng = np.random.default_rng(D + tokens)
    x_in = rc.stream(rc.stream_rows(rows, D, D), x16)
    x_in[::tokens] = 65504.0 if x16 else 1e30
    cls, pos = _f32(rng.standard_normal(D)), _f32(0.3 * rng.standard_normal(D))
    g0, b0 = rc.ln_params(D, 1)
    g1, b1 = rc.ln_params(D, 2)

    def run(mode):
        x_out = np.empty((rows, D), np.float32)
        h = np.empty((rows, D), np.float32) if mode == 0 else None
        stats = np.empty((rows, 2), np.float32) if mode == 1 else None
        q = np.empty((rows, D), np.uint8) if mode == 2 else None
        qs = np.empty((rows, D // 32), np.uint8) if mode == 2 else None
        L.check(L.lib().clipgpu_test_vision_stem(dtype, x16, mode, B, tokens, D, EPS, _p(x_in), _p(cls), _p(pos),
                                                 _p(g0), _p(b0), _p(g1), _p(b1), _p(x_out), _p(h), _p(stats), _p(q),
                                                 _p(qs)))
        return x_out, h, stats, q, qs

    seen = x_in.copy()  # the rows ln_pre sees
    seen[::tokens] = cls + pos  # f32 add, as the kernel's

    def check_x(x_out):
        if x16:
            assert np.array_equal(x_out, x_out.astype(np.float16).astype(np.float32))
            rc.check_ln16(F16, x_out, seen, g0, b0)
        else:
            rc.check_ln32(x_out, seen, g0, b0)

    check_stem_outputs(run, dtype, x16, D, g1, b1, check_x)


@pytest.mark.parametrize("x16", [0, 1], ids=["x32", "x16"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,T,D,vocab,npos", [(3, 7, 128, 50, 12), (2, 77, 512, 1000, 77), (5, 9, 1024, 33, 9)])
def test_text_stem(B, T, D, vocab, npos, dtype, x16):
    """launch_text_embed_ln: x = tok[clamp(id)] + pos[t] bit for bit (ids below 0 and past the vocabulary
    clamp; t = row % T also when pos has more rows than T), h = ln_1 of the row as stored."""
    L = _lib()
    rows = B * T
    rng = np.random.default_rng(D + T)
    ids = rng.integers(0, vocab, rows).astype(np.int64)
    ids[[1, 2, rows - 2, rows - 1]] = [0, vocab - 1, -3, vocab + 5]
    ids[T] = vocab + 5  # first token of the second sequence (t = 0 again)
    tok = rc.stream_rows(vocab, D, D + 1)
    pos = _f32(0.5 * rng.standard_normal((npos, D)))
    g1, b1 = rc.ln_params(D, 3)

    def run(mode):
        x_out = np.empty((rows, D), np.float32)
        h = np.empty((rows, D), np.float32) if mode == 0 else None
        stats = np.empty((rows, 2), np.float32) if mode == 1 else None
        q = np.empty((rows, D), np.uint8) if mode == 2 else None
        qs = np.empty((rows, D // 32), np.uint8) if mode == 2 else None
        L.check(L.lib().clipgpu_test_text_stem(dtype, x16, mode, B, T, D, vocab, npos, EPS, _p(ids), _p(tok), _p(pos),
                                               _p(g1), _p(b1), _p(x_out), _p(h), _p(stats), _p(q), _p(qs)))
        return x_out, h, stats, q, qs

    want = rc.stream(tok[np.clip(ids, 0, vocab - 1)] + pos[np.arange(rows) % T], x16)
    assert want.dtype == np.float32

    def check_x(x_out):
        assert np.array_equal(_bits(x_out), _bits(want))

    check_stem_outputs(run, dtype, x16, D, g1, b1, check_x)


@pytest.mark.parametrize("stem", ["vision", "text"])
def test_stem_refusals(stem):
    """The stems refuse what the row launchers refuse, and an MX output with D % 32 != 0."""
    L = _lib()
    for D, mode in [(1284, 0), (130, 1), (260, 2)]:
        z = np.zeros((4, D), np.float32)
        ids = np.zeros(4, np.int64)
        o, s, q = np.empty((4, D), np.float32), np.empty((4, 2), np.float32), np.empty((4, D), np.uint8)
        if stem == "vision":
            status = L.lib().clipgpu_test_vision_stem(BF16, 0, mode, 2, 2, D, EPS, _p(z), _p(z), _p(z), _p(z), _p(z), _p(z),
                                                      _p(z), _p(o), _p(o), _p(s), _p(q), _p(q))
        else:
            status = L.lib().clipgpu_test_text_stem(BF16, 0, mode, 2, 2, D, 4, 2, EPS, _p(ids), _p(z), _p(z), _p(z), _p(z),
                                                    _p(o), _p(o), _p(s), _p(q), _p(q))
        assert status == ERR_INVALID, (D, mode, status)


# ---------------------------------------------------------------- pooling

def pool(dtype, x16, B, tokens, D, x, h_bits, ids, w=None, b=None, want_pool=True, want_gather=True):
    """clipgpu_test_pool: (status, pooled, xc bits, hc bits)."""
    x = _f32(x)
    pooled = np.empty((B, D), np.float32) if want_pool else None
    xc = np.empty((B, D), np.uint16 if x16 else np.uint32) if want_gather else None
    hc = np.empty((B, D), np.uint16) if want_gather else None
    w = None if w is None else _f32(w)
    b = None if b is None else _f32(b)
    status = _lib().lib().clipgpu_test_pool(dtype, x16, B, tokens, D, _p(x), _p(h_bits) if want_gather else None, _p(ids),
                                            _p(w), _p(b), EPS, _p(pooled), _p(xc), _p(hc))
    return status, pooled, xc, hc


def bits16(n, salt):
    """n 16-bit patterns, a bijection of the index within every 65536 elements and shifted from one
    such block to the next: no two rows of a test's buffer agree, nor two elements of a row."""
    i = np.arange(n, dtype=np.uint64)
    return ((i * 40503 + (i >> 16) * 12347 + salt) & 0xFFFF).astype(np.uint16)


def finite_f16(bits):
    """16-bit patterns as normal f16 numbers (exponent fields 0 and 31 folded onto 16 and 15)."""
    e = (bits >> 10) & 31
    return np.where((e == 0) | (e == 31), bits ^ 0x4000, bits).astype(np.uint16)


def stream_bits(x, x16):
    return _f32(x).astype(np.float16).view(np.uint16) if x16 else _f32(x).view(np.uint32)


def ids_cases(B, tokens, rng):
    """(name, ids [B][tokens] or None, pooled position): the maximum id at chosen positions, lower ids
    elsewhere.  A tie takes the first position, within a lane's stride (5 and 69 = 5 + 64), across
    lanes (5 and 70), across the 64-token stride boundary (64 and 65); all zeros take position 0."""
    cases = [("cls", None, 0)]
    for name, where in [("first", [0]), ("last", [tokens - 1]), ("p70", [70]), ("tie5_70", [5, 70]),
                        ("tie64_65", [64, 65]), ("tie5_69", [5, 69]), ("tie_all", list(range(tokens)))]:
        if max(where) >= tokens:
            continue
        ids = rng.integers(1, 1000, (B, tokens)).astype(np.int64)
        ids[:, where] = 49407
        cases.append((name, ids, where[0]))
    cases.append(("zeros", np.zeros((B, tokens), np.int64), 0))
    return cases


@pytest.mark.parametrize("x16", [0, 1], ids=["x32", "x16"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,tokens,D", [(5, 77, 512), (3, 130, 128), (6, 1, 64)])
def test_pool_ln_and_gather(B, tokens, D, dtype, x16):
    """launch_pool_ln and launch_gather_pooled on the same inputs: the pooled position (CLS, or the first
    argmax of ids), pool_ln within the LayerNorm bound of that row, the gather as raw bits of it."""
    L = _lib()
    rows = B * tokens
    rng = np.random.default_rng(D + tokens)
    x = rc.stream(rc.stream_rows(rows, D, D + 5), x16)
    h = bits16(rows * D, 7).reshape(rows, D)
    w, b = rc.ln_params(D, 4)
    for name, ids, where in ids_cases(B, tokens, rng):
        if ids is not None:
            assert np.all(np.argmax(ids, 1) == where), name
        src = np.arange(B) * tokens + where
        status, pooled, xc, hc = pool(dtype, x16, B, tokens, D, x, h, ids, w, b)
        L.check(status)
        rc.check_ln16(dtype, pooled, x[src], w, b)
        assert np.array_equal(xc, stream_bits(x[src], x16)), name
        assert np.array_equal(hc, h[src]), name
    # the gather once more on a stream whose bit patterns differ element by element (every f32 pattern
    # distinct; f16 as far as 16 bits go), so that a wrong row or a short copy cannot pass
    if x16:
        xb = finite_f16(bits16(rows * D, 99)).reshape(rows, D)
        xv = xb.view(np.float16).astype(np.float32)
    else:
        xb = (0x3F000000 + np.arange(rows * D, dtype=np.uint32)).reshape(rows, D)
        xv = xb.view(np.float32)
    name, ids, where = ids_cases(B, tokens, rng)[-2]
    src = np.arange(B) * tokens + where
    status, _, xc, hc = pool(dtype, x16, B, tokens, D, xv, h, ids, want_pool=False)
    L.check(status)
    assert np.array_equal(xc, xb[src]) and np.array_equal(hc, h[src])


@pytest.mark.parametrize("x16,D", [(1, 4), (0, 4), (0, 1284), (1, 1284)])
def test_gather_pooled_widths(x16, D):
    """The gather alone at one 8-byte word per row (D = 4 on the f16 stream) and past the LayerNorm
    kernels' D cap (the gather has none); pool_ln refuses that width."""
    L = _lib()
    B, tokens = 5, 70
    rows = B * tokens
    rng = np.random.default_rng(D)
    h = bits16(rows * D, 3).reshape(rows, D)
    xb = finite_f16(bits16(rows * D, 11)).reshape(rows, D)
    x = xb.view(np.float16).astype(np.float32) if x16 else _f32(np.arange(rows * D).reshape(rows, D) - 1000.5)
    ids = rng.integers(1, 1000, (B, tokens)).astype(np.int64)
    where = np.array([0, 69, 64, 63, 7])
    ids[np.arange(B), where] = 49407
    status, _, xc, hc = pool(BF16, x16, B, tokens, D, x, h, ids, want_pool=False)
    L.check(status)
    src = np.arange(B) * tokens + where
    assert np.array_equal(xc, stream_bits(x[src], x16))
    assert np.array_equal(hc, h[src])
    if D > 1280:
        assert pool(BF16, x16, B, tokens, D, x, h, ids, np.ones(D), np.zeros(D), want_gather=False)[0] == ERR_INVALID


def test_pool_refusals():
    x = np.zeros((4, 130), np.float32)
    h = np.zeros((4, 130), np.uint16)
    assert pool(BF16, 0, 2, 2, 130, x, h, None, np.ones(130), np.zeros(130), want_gather=False)[0] == ERR_INVALID
    assert pool(BF16, 0, 2, 2, 130, x, h, None, want_pool=False)[0] == ERR_INVALID


# ---------------------------------------------------------------- MAP attention pool

def map_attention(dtype, B, N, H, D, q, kv):
    out = np.empty((B, D), np.float32)
    q, kv = _f32(q), _f32(kv)
    return _lib().lib().clipgpu_test_map_attention(dtype, B, N, H, D, _p(q), _p(kv), _p(out)), out


MAP_SHAPES = [(2, 1, 2, 64), (3, 17, 2, 8), (2, 257, 3, 72), (2, 576, 16, 72), (1, 1024, 2, 128), (2, 729, 2, 80)]


@pytest.mark.parametrize("span", [60, 100, 3])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,N,H,hd", MAP_SHAPES)
def test_map_attention(B, N, H, hd, dtype, span):
    """launch_map_attention against fp64 softmax(q.k / sqrt(hd)) @ v per (image, head): one key, fewer
    keys than V groups, N past one 256-thread stride (257), the full 1024, head dims 8 / 72 / 80 / 128;
    scores reaching +-60 and +-100 (no softmax without the max subtraction survives) and +-3 (many keys
    carry weight, so the 16-group V reduction sums them all)."""
    q, kv = rc.map_case(B, N, H, hd, dtype, span, N + hd)
    status, out = map_attention(dtype, B, N, H, H * hd, q, kv)
    _lib().check(status)
    ref = rc.map_ref(q, kv, B, N, H, hd)
    err = np.abs(out - ref)
    bound = rc.map_bound(dtype, ref, kv, H * hd)
    assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N,H,hd", [(17, 2, 8), (257, 3, 72), (1024, 2, 128)])
def test_map_attention_images_are_independent(N, H, hd, dtype):
    """Each image of a B = 3 launch equals its own B = 1 launch, bit for bit."""
    D = H * hd
    q, kv = rc.map_case(3, N, H, hd, dtype, 3, N)
    status, out = map_attention(dtype, 3, N, H, D, q, kv)
    _lib().check(status)
    for i in range(3):
        status, one = map_attention(dtype, 1, N, H, D, q, kv[i * N:(i + 1) * N])
        _lib().check(status)
        assert np.array_equal(_bits(one[0]), _bits(out[i])), i


def test_map_attention_refusals():
    """More keys than the score buffer holds, head dims past 128 or not a multiple of 8, D % H != 0."""
    for B, N, H, D in [(1, 1025, 2, 128), (1, 16, 1, 136), (1, 16, 2, 24), (1, 16, 3, 64)]:
        status, _ = map_attention(BF16, B, N, H, D, np.zeros(D), np.zeros((B * N, 2 * D)))
        assert status == ERR_INVALID, (N, H, D, status)


# ---------------------------------------------------------------- l2norm, cast

@pytest.mark.parametrize("B,E", [(1, 1), (5, 63), (7, 65), (9, 512), (3, 1152)])
def test_l2norm(B, E):
    """launch_l2norm: x / max(||x||, 1e-12) at one element, either side of a wave's 64-lane stride and at
    the embedding widths; an all-zero row gives exactly 0, a row of norm 1e-20 is divided by 1e-12."""
    L = _lib()
    for shift in range(3):
        x = rc.l2_rows(B, E, E, shift)
        out = np.empty((B, E), np.float32)
        L.check(L.lib().clipgpu_test_l2norm(B, E, _p(x), _p(out)))
        ref = rc.l2_ref(x)
        assert np.all(np.abs(out - ref) <= 32 * rc.U * np.abs(ref)), shift
        tiny = (np.arange(B) + shift) % 3 == 2
        zero, tiny = (np.arange(B) + shift) % 3 == 1, (np.arange(B) + shift) % 3 == 2
        assert np.all(out[zero] == 0)
        assert np.all(np.sqrt((out[tiny].astype(np.float64) ** 2).sum(1)) < 2e-8)  # 1e-20 / 1e-12, not 1


def cast_values(dtype):
    """4099 f32 values: random; exact ties between neighbouring 16-bit numbers of both parities;
    subnormals of the 16-bit type and ties among them; the f16 overflow threshold; infinities, NaN."""
    rng = np.random.default_rng(41 + dtype)
    shift, top = (16, 0x7F80) if dtype == BF16 else (0, 0x7C00)
    lo = rng.integers(0, top - 1, 1200).astype(np.uint32)  # finite positive 16-bit patterns, and the next one up
    lo[:200] = rng.integers(0, 0x0080 if dtype == BF16 else 0x0400, 200)  # subnormal (and 0): ties among subnormals

    def widen(p):
        return (p << 16).astype(np.uint32).view(np.float32) if dtype == BF16 else p.astype(np.uint16).view(
            np.float16).astype(np.float32)

    a, b = widen(lo), widen(lo + 1)
    ties = (a.astype(np.float64) + b.astype(np.float64)) / 2
    assert np.array_equal(ties.astype(np.float32).astype(np.float64), ties)  # exact in f32
    ties = ties.astype(np.float32)
    sub_hi = np.float32(2.0 ** -126) if dtype == BF16 else np.float32(2.0 ** -14)
    subs = (rng.uniform(0, 1, 600) * sub_hi).astype(np.float32)
    special = np.array([65504, -65504, 65519.99, 65520, -65520, 65536, 1e38, -1e38, 3.3895314e38, 3.4e38, np.inf, -np.inf,
                        np.nan, 0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -133, 2.0 ** -134,
                        2.0 ** -149], np.float32)
    fixed = np.concatenate([ties, -ties, subs, -subs, special])
    rand = (rng.standard_normal(4099 - fixed.size) * 10.0 ** rng.uniform(-6, 4, 4099 - fixed.size)).astype(np.float32)
    v = np.concatenate([fixed, rand])
    assert v.size == 4099
    return np.ascontiguousarray(v[rng.permutation(v.size)])


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_cast(dtype):
    """launch_cast_f32 (the weight upload's conversion) rounds to nearest even like round16, across the
    grid-stride loop (4099 elements), for ties, subnormals, the overflow threshold, infinities and NaN."""
    L = _lib()
    v = cast_values(dtype)
    out = np.empty(v.size, np.float32)
    L.check(L.lib().clipgpu_test_cast(dtype, v.size, _p(v), _p(out)))
    want = round16(v, dtype)
    nan = np.isnan(v)
    assert np.all(np.isnan(out[nan])) and np.all(np.isnan(want[nan])) and nan.sum() == 1
    got_b, want_b = _bits(np.nan_to_num(out)), _bits(np.nan_to_num(want))
    bad = np.flatnonzero(got_b != want_b)
    assert bad.size == 0, [(float(v[i]), hex(got_b[i]), hex(want_b[i])) for i in bad[:8]]
