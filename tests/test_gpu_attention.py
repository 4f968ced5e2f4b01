"""Kernel-level tests of the two self-attention kernels of csrc/kernels/attention.hip (attn_kernel<T, NKT>:
the whole sequence in LDS, head dim 64, N <= 256; flash_attn_kernel<T, HD>: 64-key tiles with an online
softmax, head dims 64 / 72 / 80), through clipgpu_test_attention against numpy fp64 on inputs pre-rounded
to the 16-bit type.

Every output element is held against the bound derived in tests/attention_cases.py,
  1.01 (rel16 + 2 (HD + 8) 2^-24 S) (A + |ref|) + floor V,
which tests/test_cpu_attention_bounds.py checks on the CPU: numpy-f32 emulations of both schedules stay
inside it on every case below, and six mutants (a padded key left in the softmax, a dropped last key,
scale 1/8 at head dims 72 / 80, an off-by-one causal mask, a row sum that misses the online rescale, P
rounded to bf16 in an f16 run) leave it.  The inputs (attention_cases.raw_inputs) put scores at +-60 and
+-100, move the running maximum in every key tile, or keep every real score below -5 so that a padded
key would take the mass.  The hook puts a guard after the output rows and fails if a byte of it changes.
Each test prints its worst err / bound (pytest -s).
"""
import numpy as np
import pytest

from tests import attention_cases as ac
from tests.attention_cases import BF16, F16

pytestmark = pytest.mark.gpu

ERR_INVALID = 1  # CLIPGPU_ERR_INVALID


def _lib():
    from open_clip_inference import _lib
    return _lib


def attention_rc(dtype, B, N, H, HD, causal, qkv):
    """clipgpu_test_attention: (status, out [B*N][H*HD])."""
    qkv = np.ascontiguousarray(qkv, np.float32)
    out = np.empty((max(B * N, 1), H * HD), np.float32)
    return _lib().lib().clipgpu_test_attention(dtype, B, N, H, HD, causal, qkv.ctypes.data, out.ctypes.data), out


def attention(dtype, B, N, H, HD, causal, qkv):
    status, out = attention_rc(dtype, B, N, H, HD, causal, qkv)
    _lib().check(status)
    return out


def run_case(case):
    return attention(case.dtype, case.B, case.N, case.H, case.HD, case.causal, case.qkv)


def sweep(N, HD, causal, dtype, kinds):
    """Every kind at one shape: all elements inside the bound (the message names the kind, the worst
    element and its err / bound); returns (worst err / bound, its case's name)."""
    top = (0.0, "")
    for kind, span in kinds:
        case = ac.make_case(kind, span, N, HD, causal, dtype)
        top = max(top, (case.check(run_case(case)), case.name))
    return top


@pytest.mark.parametrize("N,HD,causal,dtype", ac.WHOLE_PARAMS, ids=[ac.param_id(p) for p in ac.WHOLE_PARAMS])
def test_whole_sequence_kernel(N, HD, causal, dtype):
    """attn_kernel at both edges of every NKT instantiation (N = 32 m and 32 m + 1) and of the wave count
    (128 | 129: one wave per query tile, or 4 waves walking them), every input kind."""
    print("worst err/bound %.3f (%s)" % sweep(N, HD, causal, dtype, ac.KINDS))


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_whole_sequence_kernel_at_every_text_length(dtype):
    """Trimmed text launches every causal N from 1 to 77."""
    top = max(sweep(N, 64, 1, dtype, ac.SWEEP_KINDS) for N in ac.SWEEP_N)
    print("worst err/bound %.3f (%s)" % top)


@pytest.mark.parametrize("N,HD,causal,dtype", ac.TILED_PARAMS, ids=[ac.param_id(p) for p in ac.TILED_PARAMS])
def test_tiled_kernel(N, HD, causal, dtype):
    """flash_attn_kernel at 1 to 12 key tiles (odd and even counts through the loop unrolled by two), a
    1-key last tile (65, 129, 193, 257, 321, 577), a 1-query last block (129, 257), N below one tile at
    head dims 72 / 80, causal blocks whose diagonal tile is or is not the last; every input kind."""
    print("worst err/bound %.3f (%s)" % sweep(N, HD, causal, dtype, ac.KINDS))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N,HD", [(77, 64), (129, 64), (65, 72), (193, 72), (65, 80), (193, 80)])
def test_a_head_depends_on_its_own_rows_only(N, HD, dtype):
    """B = 3, H = 3.  With NaN everywhere but (sequence 1, head 1), that head's output equals the
    B = 1, H = 1 call on its rows bit for bit; with NaN in (sequence 1, head 1) only, every other
    (sequence, head) equals the clean run bit for bit; two identical calls give identical bits."""
    B = H = 3
    for causal in (0, 1):
        q, k, v = ac.make_inputs("spread", 3, B, N, H, HD, causal, dtype)
        clean = attention(dtype, B, N, H, HD, causal, ac.pack(q, k, v))
        assert np.array_equal(_bits(clean), _bits(attention(dtype, B, N, H, HD, causal, ac.pack(q, k, v)))), causal
        assert np.all(np.isfinite(clean))
        own = np.zeros((B, 1, H, 1), bool)
        own[1, 0, 1, 0] = True
        alone = attention(dtype, 1, N, 1, HD, causal, ac.pack(*(x[1:2, :, 1:2] for x in (q, k, v))))
        only = attention(dtype, B, N, H, HD, causal, ac.pack(*(np.where(own, x, np.float32(np.nan)) for x in (q, k, v))))
        only = ac.unpack_out(only, B, N, H, HD)
        assert np.array_equal(_bits(only[1, :, 1]), _bits(alone)), causal
        assert np.array_equal(_bits(only[1, :, 1]), _bits(ac.unpack_out(clean, B, N, H, HD)[1, :, 1])), causal
        rest = attention(dtype, B, N, H, HD, causal, ac.pack(*(np.where(own, np.float32(np.nan), x) for x in (q, k, v))))
        rest = ac.unpack_out(rest, B, N, H, HD)
        assert np.all(np.isnan(rest[1, :, 1])), causal
        others = np.broadcast_to(~own, rest.shape)
        assert np.array_equal(_bits(rest[others]), _bits(ac.unpack_out(clean, B, N, H, HD)[others])), causal


def test_refusals():
    """launch_attention's own refusal (a head dim no kernel is built for) and the hook's (no heads, no
    keys, no sequences) come back as CLIPGPU_ERR_INVALID, not as a device error, and the next call is
    clean.  (D % H != 0 cannot be put through this hook: it passes D = H * HD.)"""
    for B, N, H, HD in [(2, 16, 2, 96), (2, 300, 2, 96), (2, 16, 2, 56), (2, 16, 0, 64), (2, 0, 2, 64), (0, 16, 2, 64)]:
        status, _ = attention_rc(BF16, B, N, H, HD, 0, np.zeros((max(B * N, 1), 3 * max(H, 1) * HD), np.float32))
        assert status == ERR_INVALID, (B, N, H, HD, status)
    case = ac.make_case("spread", 3, 16, 64, 0, BF16)
    case.check(run_case(case))
