"""Everything that produces MX-fp8 bytes, and the MX GEMM as the engine launches it, held per byte
(tests/mx_cases.py; tests/test_cpu_mx_cases.py checks the cases, bounds and mutants on the CPU).

  exact (==):   EPI_STOREQ without activation (storeq_case: t = A.W^T + bias is exact in f32 in any order),
                on every shape, tile and type, through the persistent walk (a block takes three tiles), the
                launcher's row chunks and padded pitches; the 16-bit, f32 and f16-stream epilogues through the
                same walk and chunks; the stems' MX bytes against launch_ln_rows' on both streams.
  per element,  LayerNorm with MX output (delta = rowwise_cases.f32bound) and EPI_STOREQ with an activation
  in a derived  (delta = mx_cases.act_delta): check_mx holds every scale byte and every code to what
  interval:     [ref - delta, ref + delta] allows; the share of inputs that leaves two choices is capped on the
                CPU and printed here (-s).
  still bounded (tests/test_gpu_mx.py, test_gpu_gemm.py): the scaled MFMA's accumulation on random operands,
                2^-12 sum |a||w|.
"""
import numpy as np
import pytest

from tests import gemm_cases as gc
from tests import mx_cases as mc
from tests.gemm_cases import BF16, F16
from tests.test_gpu_gemm import assert_same, run_mx
from tests.test_gpu_rowwise import ln_rows

pytestmark = pytest.mark.gpu

ERR_INVALID = 1  # CLIPGPU_ERR_INVALID
FILL = 0xA5      # what the output buffers hold before a launch: every byte of [M][N] and [M][N/32] is written
TYPES = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
MX_TILES = [0, 2, 3]
TILE_IDS = ["auto", "mx256x128", "mx128x128"]
SHAPE_IDS = ["x".join(map(str, s)) for s in mc.STOREQ_SHAPES]


def _lib():
    from open_clip_inference import _lib
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


@pytest.fixture(params=MX_TILES, ids=TILE_IDS)
def mx_tile(request, monkeypatch):
    monkeypatch.setenv("CLIPGPU_TEST_TILE", str(request.param))
    return request.param


def report(what, amb):
    print(f"\n[mx] {what}: ambiguous blocks {amb[0]:.4%} elements {amb[1]:.4%}")


# ---- a. LayerNorm with MX output -------------------------------------------------------------------------
@pytest.mark.parametrize("x16", [0, 1], ids=["x32", "x16"])
@TYPES
@pytest.mark.parametrize("D", mc.LN_DIMS)
def test_ln_mx_every_scale_and_code(D, dtype, x16):
    """launch_ln_rows' MX output (store_row_mx) on both streams, one block and every NV: every scale byte and
    code within what 64 roundings of the f32 LayerNorm allow around the fp64 LayerNorm of the stored row."""
    c = mc.ln_case(D, x16)
    _, _, q, qs = ln_rows(dtype, x16, c.x, c.w, c.b, mx=True)
    report(f"LN D {D} x16 {x16}", mc.check_mx(q, qs, c.ref, c.delta, f"LN-MX D {D} x16 {x16}"))


# ---- c. the quantizing epilogue ----------------------------------------------------------------------------
def storeq_rc(dtype, act, c, tile, lda=None, ldw=None, ldo=None, ldos=None, outs=True, pad=0x7F):
    """clipgpu_test_gemm_mx_q_at on the case at the given pitches (default dense): (status, outq [M][ldo],
    outs [M][ldos]), both FILL before the launch; the operands' pad bytes hold the NaN code."""
    M, N, K = c.M, c.N, c.K
    lda, ldw, ldo, ldos = lda or K, ldw or K, ldo or N, ldos or N // 32
    aq, wq = np.full((M, lda), pad, np.uint8), np.full((N, ldw), pad, np.uint8)
    aq[:, :K], wq[:, :K] = c.aq, c.wq
    outq, outs_ = np.full((M, ldo), FILL, np.uint8), np.full((M, ldos), FILL, np.uint8)
    rc = _lib().lib().clipgpu_test_gemm_mx_q_at(dtype, act, M, N, K, lda, ldw, ldo, ldos, tile, _p(aq), _p(c.as_),
                                               _p(wq), _p(c.ws), _p(c.bias), _p(outq), _p(outs_) if outs else None)
    return rc, outq, outs_


def storeq_at(dtype, act, c, tile, **kw):
    rc, q, s = storeq_rc(dtype, act, c, tile, **kw)
    _lib().check(rc)
    return q, s


def check_storeq(c, act, q, s, what):
    """Bytes of EPI_STOREQ against the case: == without activation, the interval check with one."""
    if act == 0:
        mc.assert_bytes(s, c.rs, f"{what}: scales")
        mc.assert_bytes(q, c.rq, f"{what}: codes")
        return 0.0, 0.0
    return mc.check_mx(q, s, c.z(act), c.delta(act), what)


@TYPES
@pytest.mark.parametrize("M,N,K", mc.STOREQ_SHAPES, ids=SHAPE_IDS)
def test_storeq_bytes(M, N, K, dtype, mx_tile):
    """clipgpu_test_gemm_mx mode 3 (as every default fp8 engine runs c_fc) on exact operands: M and N tails on
    both tiles, one K step, a row past a 32-row MFMA group, the pruned tail's M = 5 and 1; output blocks over
    at least four scales with an all-zero block; the block maximum in either lane of the xmax32 exchange;
    values exactly between two codes.  Without activation the bytes are the oracle's; with one, every byte
    is within act_delta's interval."""
    L = _lib()
    c = mc.storeq_case(M, N, K)
    for act in (0, 1, 2, 3):
        q, s = np.full((M, N), FILL, np.uint8), np.full((M, N // 32), FILL, np.uint8)
        L.check(L.lib().clipgpu_test_gemm_mx(dtype, 3, act, M, N, K, _p(c.aq), _p(c.as_), _p(c.wq), _p(c.ws),
                                             _p(c.bias), None, None, _p(q), _p(s)))
        amb = check_storeq(c, act, q, s, f"{M}x{N}x{K} act {act} tile {mx_tile}")
        if act:
            report(f"storeq {M}x{N}x{K} act {act}", amb)


# ---- d. the persistent walk ----------------------------------------------------------------------------------
def test_persistent_walk_takes_three_tiles_per_block():
    """More than two resident rounds of tiles on both MX tiles: t += t_stride twice, the bias slice parity
    reused by the third tile, read_step0 for the next tile, the wait accounting after a full tile's epilogue;
    M and N tails.  The 16-bit store (the QKV site), the f16 stream (c_proj), and the quantizing epilogue
    (c_fc) without activation are exact; QuickGELU goes through the interval check."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, K = mc.walk_shape(cus)
    for tile in (2, 3):
        per = mc.walk_tiles_per_block(M, N, tile, cus)
        assert max(per) >= 3, (tile, cus, max(per))
    c = gc.mx_case(M, N, K)
    ops = (c.aq, c.as_, c.wq, c.ws)
    for mode, dtype in ((0, BF16), (4, BF16)):
        ref = c.ref(mode, dtype)
        for tile in MX_TILES:
            assert_same(run_mx(dtype, mode, ops, c.bias, c.x(mode), tile), ref, f"mode {mode} tile {tile}")
    s = mc.storeq_case(M, N, K)
    for tile in MX_TILES:
        check_storeq(s, 0, *storeq_at(BF16, 0, s, tile), f"STOREQ tile {tile}")
    for tile in MX_TILES:
        report(f"walk STOREQ QuickGELU tile {tile}",
               check_storeq(s, 1, *storeq_at(BF16, 1, s, tile), f"STOREQ QuickGELU tile {tile}"))


# ---- e. row chunks -----------------------------------------------------------------------------------------------
def test_row_chunks_are_bit_invisible():
    """launch_gemm_mx's row-chunk loop (its own pointer arithmetic on A, its scales, the output and the
    output's scales; in the product only past 2^31 operand bytes) under the test cap of 256 rows: chunks of
    256, 256 and 188 rows equal the one launch bit for bit, and the exact reference, for every epilogue."""
    L = _lib()
    M, N, K = mc.CHUNK_SHAPE
    c, s = gc.mx_case(M, N, K), mc.storeq_case(M, N, K)
    ops = (c.aq, c.as_, c.wq, c.ws)

    def run_all(tile):
        outs = [run_mx(BF16, mode, ops, c.bias, c.x(mode), tile) for mode in gc.MX_MODES]
        return outs + [storeq_at(BF16, act, s, tile) for act in (0, 1)]

    for tile in MX_TILES:
        whole = run_all(tile)
        L.check(L.lib().clipgpu_test_gemm_chunk_rows(256))
        try:
            chunked = run_all(tile)
        finally:
            L.check(L.lib().clipgpu_test_gemm_chunk_rows(0))
        for mode, a, b in zip(gc.MX_MODES, whole, chunked):
            assert_same(b, a, f"mode {mode} tile {tile}: chunked against whole")
            assert_same(b, c.ref(mode, BF16), f"mode {mode} tile {tile}: chunked")
        for act, a, b in zip((0, 1), whole[-2:], chunked[-2:]):
            mc.assert_bytes(b[0], a[0], f"STOREQ act {act} tile {tile}: chunked codes against whole")
            mc.assert_bytes(b[1], a[1], f"STOREQ act {act} tile {tile}: chunked scales against whole")
            check_storeq(s, act, *b, f"STOREQ act {act} tile {tile}: chunked")
    # a cap below one 256-row tile leaves no whole tile to chunk by: refused
    L.check(L.lib().clipgpu_test_gemm_chunk_rows(100))
    try:
        assert storeq_rc(BF16, 0, s, 3)[0] == ERR_INVALID
    finally:
        L.check(L.lib().clipgpu_test_gemm_chunk_rows(0))


# ---- f. pitches and refusals -----------------------------------------------------------------------------------------
PITCH_SHAPE = mc.STOREQ_SHAPES[0]


@TYPES
@pytest.mark.parametrize("tile", MX_TILES, ids=TILE_IDS)
def test_storeq_padded_pitches(tile, dtype):
    """lda = ldw = K + 16 with the NaN code in the pad bytes, ldo = N + 16, ldos = N/32 + 3: the bytes of the
    dense run, and the outputs' pad bytes keep what they held."""
    M, N, K = PITCH_SHAPE
    c = mc.storeq_case(M, N, K)
    for act in (0, 2):
        dq, ds = storeq_at(dtype, act, c, tile)
        q, s = storeq_at(dtype, act, c, tile, lda=K + 16, ldw=K + 16, ldo=N + 16, ldos=N // 32 + 3)
        mc.assert_bytes(q[:, :N], dq, f"act {act}: codes against the dense run")
        mc.assert_bytes(s[:, :N // 32], ds, f"act {act}: scales against the dense run")
        assert np.all(q[:, N:] == FILL) and np.all(s[:, N // 32:] == FILL), f"act {act}: pad bytes written"
        check_storeq(c, act, dq, ds, f"act {act} dense")


def test_storeq_refusals():
    """EPI_STOREQ's pitch contract (kernels.hpp): each violation is CLIPGPU_ERR_INVALID before anything is
    launched (both buffers keep their bytes), and a valid launch afterwards gives the right bytes."""
    M, N, K = PITCH_SHAPE
    c = mc.storeq_case(M, N, K)
    for what, kw in [("ldo % 16", dict(ldo=N + 8)), ("ldo < N", dict(ldo=N - 16)), ("ldos < N/32", dict(ldos=N // 32 - 1)),
                     ("outs == nullptr", dict(outs=False))]:
        rc, q, s = storeq_rc(BF16, 0, c, 3, **kw)
        assert rc == ERR_INVALID, (what, rc)
        assert np.all(q == FILL) and np.all(s == FILL), what
    check_storeq(c, 0, *storeq_at(BF16, 0, c, 3), "a valid launch after the refusals")

