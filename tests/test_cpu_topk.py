"""The embedding index without a GPU: the search's order key (csrc/kernels/topk_key.hpp, through
clipgpu_test_topk_key) and the create-time argument errors, raised before any device call."""
import ctypes

import numpy as np
import pytest


def key(score, index):
    from open_clip_inference import _lib
    k = ctypes.c_uint64()
    _lib.check(_lib.lib().clipgpu_test_topk_key(float(np.float32(score)), int(index), ctypes.byref(k)))
    return k.value


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


ASCENDING = [-np.inf, -3.0e38, -100.0, -1.0, -1.1754944e-38, f32(0x80000001), -0.0, 0.0, f32(0x00000001),
             1.1754944e-38, 0.5, 1.0, 100.0, 3.0e38, np.inf]


def test_key_orders_as_the_scores_do():
    ks = [key(s, 7) for s in ASCENDING]
    for a, b, ka, kb in zip(ASCENDING, ASCENDING[1:], ks, ks[1:]):
        assert ka <= kb, (a, b)
        if np.float32(a) != np.float32(b):  # every neighbouring pair but (-0.0, +0.0)
            assert ka < kb, (a, b)
    assert key(-0.0, 5) == key(0.0, 5)
    assert key(f32(0x80000001), 5) < key(-0.0, 5)  # the negative denormal is not flushed into the zeros


def test_key_breaks_ties_by_ascending_index():
    for s in (-np.inf, -1.5, -0.0, 0.0, 2.25, np.inf):
        assert key(s, 0) > key(s, 1) > key(s, 1000) > key(s, 2**31 - 1)
    # the score decides before the index does
    assert key(1.0, 2**31 - 1) > key(np.nextafter(np.float32(1.0), np.float32(0.0)), 0)
    # the key is (score part) << 32 | ~index
    assert key(1.0, 3) & 0xFFFFFFFF == (~3) & 0xFFFFFFFF


def test_nan_ranks_below_minus_infinity():
    lowest = key(-np.inf, 2**31 - 1)
    for bits in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF):
        assert key(f32(bits), 0) < lowest, hex(bits)
        assert key(f32(bits), 0) > key(f32(bits), 1)  # NaNs among themselves: by index
        assert key(f32(bits), 2**31 - 1) > 0  # 0 is the empty slot, below every real entry


@pytest.mark.parametrize("E,capacity,null_out,msg", [(0, 8, False, "embedding dim must be a multiple of 16"),
                                                     (24, 8, False, "embedding dim must be a multiple of 16"),
                                                     (64, 0, False, "capacity must be positive"),
                                                     (64, 8, True, "NULL out")])
def test_create_argument_errors(E, capacity, null_out, msg):
    from open_clip_inference import _lib
    from open_clip_inference.error import ClipError
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.clipgpu_index_create(0, E, capacity, None if null_out else ctypes.byref(h))
    assert rc == 1  # CLIPGPU_ERR_INVALID
    assert msg in L.clipgpu_last_error().decode()
    assert not h.value
    if not null_out:
        from open_clip_inference import EmbeddingIndex
        with pytest.raises(ClipError, match=msg):
            EmbeddingIndex(E, capacity)


def test_span_hook_takes_multiples_of_64():
    from open_clip_inference import _lib
    L = _lib.lib()
    assert L.clipgpu_test_topk_span_cols(100) == 1 and b"multiple of 64" in L.clipgpu_last_error()
    assert L.clipgpu_test_topk_span_cols(-64) == 1
    assert L.clipgpu_test_topk_span_cols(128) == 0
    assert L.clipgpu_test_topk_span_cols(0) == 0
