"""The GEMM family (kernels/gemm.hip, kernels/gemm_mx.hip) at the launch parameters the engine uses,
held to exact references.

Operands are small integers (tests/gemm_cases.py: the f32 accumulator is then exact in any order and the
epilogue's f32 adds and single rounding are reproduced by numpy bit for bit), so every comparison here
is np.array_equal: every built tile and the skinny / general kernels, both 16-bit types, every epilogue
(16-bit store, f32 and f16 residual stream, f32 store, the patch epilogue with and without a class token
and a bias), the tile order and wave priority of the engine's sites (GemmParams.group / prio), padded
row pitches, the row-chunked path, the MX-fp8 GEMM's epilogues -- and the launchers' refusals.
tests/test_cpu_gemm_cases.py checks the references, and that the inputs tell a wrong result from a
right one, without a GPU.
"""
import numpy as np
import pytest

from oracle import mx_ref
from tests import gemm_cases as gc
from tests.gemm_cases import BF16, F16, GENERAL, SENTINEL, SKINNY, TILES, TILE_IDS

pytestmark = pytest.mark.gpu

ERR_INVALID = 1  # CLIPGPU_ERR_INVALID
TYPES = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
EACH_TILE = pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)


def _lib():
    from open_clip_inference import _lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def gemm_at_rc(dtype, mode, M, N, K, A, W, bias, out, tile, group=0, prio=0, act=0):
    """clipgpu_test_gemm_at on A [M][lda], W [N][ldw], out [M][ldo] (in place): the status."""
    assert A.dtype == W.dtype == out.dtype == np.float32 and A.flags.c_contiguous and W.flags.c_contiguous
    assert out.flags.c_contiguous and A.shape[0] == M and W.shape[0] == N and out.shape[0] == M
    bias = None if bias is None else np.ascontiguousarray(bias, np.float32)
    return _lib().lib().clipgpu_test_gemm_at(dtype, mode, act, M, N, K, A.shape[1], W.shape[1], out.shape[1], tile,
                                            group, prio, _ptr(A), _ptr(W), _ptr(bias), _ptr(out))


def run_dense(c, dtype, mode, tile, bias=True, group=0, prio=0):
    """The case at dense pitches: the output [M][N]."""
    x = c.x(mode)
    out = np.full((c.M, c.N), SENTINEL, np.float32) if x is None else x.copy()
    _lib().check(gemm_at_rc(dtype, mode, c.M, c.N, c.K, c.A, c.W, c.bias if bias else None, out, tile, group, prio))
    return out


def assert_same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        r, col = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {ref.size} elements differ, first at [{r}][{col}]: "
                             f"got {got[r, col]!r}, want {ref[r, col]!r}; rows {np.unique(bad[:, 0])[:8]}, "
                             f"columns {np.unique(bad[:, 1])[:8]}")


# ---- every tile, type and epilogue -------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("M,N,K", gc.SHAPES, ids=["x".join(map(str, s)) for s in gc.SHAPES])
def test_every_tile_and_epilogue_is_exact(M, N, K, dtype):
    """Modes 0 (no activation), 1, 2, 3 on every built tile, the general form and (where it applies) the
    skinny kernel, and the launcher's own pick.  700 x 520: 3-5 row and column panels with M and N tails on
    every tile."""
    c = gc.gemm_case(M, N, K)
    for mode in gc.MODES:
        ref = c.ref(mode, dtype)
        for tile in [0] + gc.tiles_for(M, N, K):
            assert_same(run_dense(c, dtype, mode, tile), ref, f"mode {mode} tile {tile}")
    ref = c.ref(2, dtype, bias=False)
    for tile in gc.tiles_for(M, N, K):
        assert_same(run_dense(c, dtype, 2, tile, bias=False), ref, f"mode 2 without a bias, tile {tile}")


@TYPES
@pytest.mark.parametrize("M,N,K", gc.GENERAL_SHAPES, ids=["N100", "K64"])
def test_shapes_only_the_general_form_takes(M, N, K, dtype):
    """A 16-bit output row of 100 elements and a single K-step run the general form whatever the tile."""
    c = gc.gemm_case(M, N, K)
    ref = c.ref(0, dtype)
    for tile in [0, 15, 26, GENERAL]:
        assert_same(run_dense(c, dtype, 0, tile), ref, f"tile {tile}")


@EACH_TILE
def test_a_second_rounding_would_show(tile):
    """The case whose bf16 results nearly all sit where result -> f16 -> bf16 differs from one rounding."""
    c = gc.rounding_case()
    assert_same(run_dense(c, BF16, 0, tile), c.ref(0, BF16), f"tile {tile}")


# ---- tile order and priority ---------------------------------------------------------------------------
@EACH_TILE
def test_tile_order_and_priority_never_change_the_result(tile):
    """GemmParams.group in {0 (the kernels' 8), 1 (the engine's QKV / c_proj), 3} x prio in {0, 1 (the
    vision tower)}: each against the exact reference, on the f16 residual stream (bf16 operands) and the
    16-bit store (f16 operands)."""
    c = gc.gemm_case(*gc.SHAPES[0])
    for dtype, mode in ((BF16, 3), (F16, 0)):
        ref = c.ref(mode, dtype)
        for group in (0, 1, 3):
            for prio in (0, 1):
                assert_same(run_dense(c, dtype, mode, tile, group=group, prio=prio), ref,
                            f"mode {mode} group {group} prio {prio}")


@EACH_TILE
def test_persistent_walk_in_the_engines_order(tile):
    """More tiles than resident blocks (each block walks several), group = 1 and prio = 1, M and N tails."""
    c = gc.gemm_case(*gc.WALK_SHAPE)
    ref = c.ref(gc.WALK_MODE, gc.WALK_TYPE)
    assert_same(run_dense(c, gc.WALK_TYPE, gc.WALK_MODE, tile, group=1, prio=1), ref, f"tile {tile}")


@pytest.mark.parametrize("M,N,K", [(700, 520, 512), (77, 2304, 768)])
def test_folded_layernorm_gemm_in_the_engines_order(M, N, K):
    """EPI_LNF with group = 1, prio = 1 (the engine's QKV site on a vision tower) is bit-equal to the
    plain launch, whose fp64 bound test_gpu_kernels.test_layernorm_folded_gemm holds."""
    from tests.test_gpu_kernels import lnf_case, run_lnf
    L = _lib()
    x, _, _, _, _, wf, cs, bp = lnf_case(M, N, K, M + N)
    args = [np.ascontiguousarray(a, np.float32) for a in (x, wf, cs, bp)]
    for tile in TILES:
        want = run_lnf(BF16, 1, x, wf, cs, bp, 1e-5, tile)
        got = np.empty((M, N), np.float32)
        L.check(L.lib().clipgpu_test_gemm_lnf_at(BF16, 1, M, N, K, *[a.ctypes.data for a in args], 1e-5, tile, 1, 1,
                                                 got.ctypes.data))
        assert_same(got, want, f"tile {tile}")


# ---- row pitches ---------------------------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("tile", TILES + [GENERAL], ids=TILE_IDS + ["general"])
def test_padded_pitches(tile, dtype):
    """lda = K + 8, ldw = K + 24, ldo = N + 8: NaN in the operands' pad columns never reaches a result, and
    the output's pad columns keep their sentinel."""
    M, N, K = gc.PITCH_SHAPE
    c = gc.gemm_case(M, N, K)
    A = gc.padded(c.A, K + gc.PAD_A, np.nan)
    W = gc.padded(c.W, K + gc.PAD_W, np.nan)
    for mode in gc.MODES:
        x = c.x(mode)
        out = np.full((M, N + gc.PAD_O), SENTINEL, np.float32)
        if x is not None:
            out[:, :N] = x
        _lib().check(gemm_at_rc(dtype, mode, M, N, K, A, W, c.bias, out, tile, group=1, prio=1))
        assert_same(out[:, :N], c.ref(mode, dtype), f"mode {mode}")
        assert np.all(out[:, N:] == SENTINEL), f"mode {mode}: pad columns written"


# ---- the patch GEMM ------------------------------------------------------------------------------------
def run_patch(c, dtype, x16, tile, bias=True):
    x = c.x0.copy()
    b = c.bias if bias else None
    _lib().check(_lib().lib().clipgpu_test_patch_gemm(dtype, x16, c.cls, c.B, c.G, c.Kp, c.D, tile, _ptr(c.rows),
                                                      _ptr(c.W), _ptr(b), _ptr(c.pos), _ptr(x)))
    return x


@TYPES
@pytest.mark.parametrize("x16", [0, 1], ids=["x32", "x16"])
@pytest.mark.parametrize("cls", [0, 1], ids=["nocls", "cls"])
def test_patch_epilogue(cls, x16, dtype):
    """EPI_PATCH / EPI_PATCH16 with and without a class token and a conv bias, on every pipelined tile: 40
    images of 9 patches (image boundaries inside every tile, at odd rows), D with and without an N tail, and
    one patch per image.  Row b (G^2 + cls) + cls + p gets acc + bias + pos[cls + p]; the class rows keep
    what they held."""
    for B, G, Kp, D in gc.PATCH_SHAPES:
        c = gc.patch_case(cls, B, G, Kp, D)
        for bias in (True, False):
            ref = c.ref(x16, bias)
            for tile in TILES:
                assert_same(run_patch(c, dtype, x16, tile, bias), ref, f"B {B} G {G} D {D} bias {bias} tile {tile}")


@pytest.mark.parametrize("cls", [0, 1], ids=["nocls", "cls"])
def test_patch_epilogue_in_row_chunks(cls):
    """The same through launch_gemm's row-chunked path: a cap of 256 rows gives chunks of 252 = 28 whole
    images, whose output rows start at token row 28 (9 + cls)."""
    L = _lib()
    B, G, Kp, D = gc.PATCH_SHAPES[1]
    c = gc.patch_case(cls, B, G, Kp, D)
    L.check(L.lib().clipgpu_test_gemm_chunk_rows(256))
    try:
        for x16 in (0, 1):
            for tile in (0, 15, 26):
                assert_same(run_patch(c, BF16, x16, tile), c.ref(x16), f"x16 {x16} tile {tile}")
    finally:
        L.check(L.lib().clipgpu_test_gemm_chunk_rows(0))


# ---- MX-fp8 --------------------------------------------------------------------------------------------
def mx_at_rc(dtype, mode, act, M, N, K, aq, as_, wq, ws, bias, resid, out, tile):
    for a in (aq, as_, wq, ws):
        assert a.dtype == np.uint8 and a.flags.c_contiguous
    return _lib().lib().clipgpu_test_gemm_mx_at(dtype, mode, act, M, N, K, aq.shape[1], wq.shape[1], tile, _ptr(aq),
                                               _ptr(as_), _ptr(wq), _ptr(ws), _ptr(bias), _ptr(resid), _ptr(out))


def run_mx(dtype, mode, ops, bias, resid, tile, act=0):
    aq, as_, wq, ws = ops
    M, K = aq.shape
    N = wq.shape[0]
    out = np.full((M, N), SENTINEL, np.float32)
    bias = None if bias is None else np.ascontiguousarray(bias, np.float32)
    resid = None if resid is None else np.ascontiguousarray(resid, np.float32)
    _lib().check(mx_at_rc(dtype, mode, act, M, N, K, aq, as_, wq, ws, bias, resid, out, tile))
    return out


@TYPES
@pytest.mark.parametrize("M,N,K", gc.MX_SHAPES)
def test_mx_epilogues_are_exact_on_integers(M, N, K, dtype):
    """Integer operands under one block scale (exact in MX-fp8): the scaled MFMA sums them exactly
    (tools/mx_diag.py's observation, confirmed at these shapes by this test), and the epilogues -- 16-bit
    store, f32 and f16 residual stream (what every default fp8 engine runs for c_proj), f32 store -- are
    the 16-bit GEMM's: equal to the reference bit for bit, on both MX tiles and the launcher's pick."""
    c = gc.mx_case(M, N, K)
    ops = (c.aq, c.as_, c.wq, c.ws)
    for mode in gc.MX_MODES:
        ref = c.ref(mode, dtype)
        for tile in gc.MX_TILES:
            assert_same(run_mx(dtype, mode, ops, c.bias, c.x(mode), tile), ref, f"mode {mode} tile {tile}")


def mx_bound(ops, bias, resid):
    aq, as_, wq, ws = ops
    b = np.abs(mx_ref.dequantize(aq, as_)) @ np.abs(mx_ref.dequantize(wq, ws)).T + np.abs(bias)
    return b if resid is None else b + np.abs(resid)


@pytest.mark.parametrize("tile", gc.MX_TILES, ids=["auto", "mx256x128", "mx128x128"])
def test_mx_f16_stream_and_f16_output_on_random_operands(tile):
    """Random MX operands (as tests/test_gpu_mx.py) at its bounds: 2^-12 of sum |a||w| (+ |bias| + |resid|)
    for the scaled MFMA's accumulation, plus one rounding of the output type (2^-11 |ref| for f16)."""
    M, N, K = 700, 512, 1024
    ops = gc.mx_random_operands(M, N, K, 5)
    rng = np.random.default_rng(6)
    bias = rng.standard_normal(N).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float16).astype(np.float32)
    ref = mx_ref.mx_gemm_ref(*ops, bias)
    for dtype in (BF16, F16):  # mode 4: the f16 stream, whatever the operand type's 16-bit side
        out = run_mx(dtype, 4, ops, bias, resid, tile)
        r = ref + resid
        assert np.all(np.abs(out - r) <= 2.0 ** -11 * np.abs(r) + 2.0 ** -12 * mx_bound(ops, bias, resid))
    out = run_mx(F16, 0, ops, bias, None, tile)
    assert np.all(np.abs(out - ref) <= 2.0 ** -11 * np.abs(ref) + 2.0 ** -12 * mx_bound(ops, bias, None))
    out = run_mx(F16, 2, ops, bias, None, tile)
    assert np.all(np.abs(out - ref) <= 2.0 ** -12 * mx_bound(ops, bias, None))


@pytest.mark.parametrize("tile", gc.MX_TILES, ids=["auto", "mx256x128", "mx128x128"])
def test_mx_block_scales_spread_along_k(tile):
    """A's block scales run over 2^-6 .. 2^6 along K (W's the other way, so every block's products weigh the
    same): the per-block scale pairing of the MFMA, at the 2^-12 sum |a||w| bound."""
    M, N, K = 300, 160, 1024
    ops = gc.mx_random_operands(M, N, K, 9, k_spread=True)
    assert len(np.unique(ops[1])) >= 13 and len(np.unique(ops[3])) >= 13
    bias = np.random.default_rng(10).standard_normal(N).astype(np.float32)
    out = run_mx(BF16, 2, ops, bias, None, tile)
    ref = mx_ref.mx_gemm_ref(*ops, bias)
    assert np.all(np.abs(out - ref) <= 2.0 ** -12 * mx_bound(ops, bias, None) + 1e-30)


# ---- refusals ------------------------------------------------------------------------------------------
def test_launch_gemm_refusals():
    """The launcher's contract (kernels.hpp): each violation comes back as CLIPGPU_ERR_INVALID before
    anything is launched -- the output buffer keeps its sentinel -- and a valid launch afterwards gives the
    right bits."""
    M, N, K = gc.PITCH_SHAPE
    c = gc.gemm_case(M, N, K)

    def refused(what, mode=2, tile=15, A=c.A, W=c.W, bias=c.bias, ldo=N, n=N, k=K, m=M):
        out = np.full((m, ldo), SENTINEL, np.float32)
        rc = gemm_at_rc(BF16, mode, m, n, k, np.ascontiguousarray(A[:m]), W, bias, out, tile)
        assert rc == ERR_INVALID, (what, rc)
        assert np.all(out == SENTINEL), what

    refused("lda = K + 4", A=gc.padded(c.A, K + 4, 0.0))
    refused("ldw = K + 4", W=gc.padded(c.W, K + 4, 0.0))
    refused("lda < K", A=np.ascontiguousarray(c.A[:, :K - 8]))
    refused("ldw < K", W=np.ascontiguousarray(c.W[:, :K - 8]))
    refused("ldo < N", ldo=N - 8)
    refused("ldo < N, 16-bit output", mode=0, ldo=N - 8)
    refused("ldo % 4 with an f32 output", ldo=N + 2)
    refused("ldo % 4 with an f32 residual", mode=1, ldo=N + 2)
    refused("ldo % 4 with an f16 stream", mode=3, ldo=N + 2)
    refused("bias with N % 4", W=np.ascontiguousarray(c.W[:N - 2]), bias=c.bias[:N - 2], n=N - 2, ldo=N)
    refused("the skinny kernel at M = 300", tile=SKINNY, m=300)
    refused("an unbuilt tile", tile=4)
    refused("K % 64", A=np.ascontiguousarray(c.A[:, :K - 32]), W=np.ascontiguousarray(c.W[:, :K - 32]), k=K - 32)
    # the patch epilogue has no general form
    p = gc.patch_case(1, *gc.PATCH_SHAPES[0])
    x = p.x0.copy()
    rc = _lib().lib().clipgpu_test_patch_gemm(BF16, 0, p.cls, p.B, p.G, p.Kp, p.D, GENERAL, _ptr(p.rows), _ptr(p.W),
                                              _ptr(p.bias), _ptr(p.pos), _ptr(x))
    assert rc == ERR_INVALID and np.all(x == SENTINEL)
    assert_same(run_dense(c, BF16, 2, 15), c.ref(2, BF16), "a valid launch after the refusals")
    assert_same(run_patch(p, BF16, 0, 15), p.ref(0), "a valid patch launch after the refusals")


def test_launch_gemm_mx_refusals():
    M, N, K = gc.MX_SHAPES[1]
    c = gc.mx_case(M, N, K)
    out = np.full((M, N), SENTINEL, np.float32)
    pad = np.zeros((M, K + 8), np.uint8)
    pad[:, :K] = c.aq
    for what, kw in [("the unbuilt 256x256 tile", dict(tile=1)), ("lda % 16", dict(aq=pad)),
                     ("an activation on the residual epilogue", dict(mode=1, act=1, resid=c.resid)),
                     ("an activation on the f16 stream", dict(mode=4, act=2, resid=c.resid16))]:
        a = dict(mode=2, act=0, aq=c.aq, resid=None, tile=3)
        a.update(kw)
        rc = mx_at_rc(BF16, a["mode"], a["act"], M, N, K, a["aq"], c.as_, c.wq, c.ws, c.bias, a["resid"], out,
                      a["tile"])
        assert rc == ERR_INVALID, (what, rc)
        assert np.all(out == SENTINEL), what
    ops = (c.aq, c.as_, c.wq, c.ws)
    assert_same(run_mx(BF16, 2, ops, c.bias, None, 3), c.ref(2, BF16), "a valid launch afterwards")
