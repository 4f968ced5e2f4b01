"""End-to-end parity of the HIP engine vs the CPU oracle (fp64 restatement of the
reference's ONNX graphs, pinned against HF transformers — tests/test_cpu_oracle.py).

Tolerance (north_star): cosine(GPU, oracle) >= 0.9999 per embedding row, and the
GPU rows are unit-norm to 1e-5.  Weights are the seeded synthetic set (identical
bits on both sides, tests/test_cpu_host.py::test_synth_matches_oracle).
"""
import ctypes
from ctypes import c_int

import numpy as np
import pytest

from oracle import clip_ref, weights
from oracle.model_spec import (LONG_H14_CFG, LONG_SIGLIP_CFG, OPENAI_MEAN, OPENAI_STD, SIGLIP_MEAN, SIGLIP_STD,
                               SO400M_16_SIGLIP2_384_CFG, TINY_CFG, TINY_H14_CFG, TINY_SIGLIP_CFG, VIT_B_32_CFG,
                               VIT_H_14_378_CFG)
from tests.helpers import COS_TOL, make_model_dir, normalized_pixels, specs

pytestmark = pytest.mark.gpu

BUILT_TILES = [2, 3, 13, 14, 15, 17, 18, 26]  # kernels.hpp kGemmTiles (test_cpu_abi checks the list)

_CACHE = {}


def oracle_vision(cfg, seed, px):
    v, _ = specs(cfg)
    key = ("v", id(cfg), seed)
    if key not in _CACHE:
        _CACHE[key] = weights.vision_weights(v, seed)
    return clip_ref.encode_image(_CACHE[key], v, px)


def oracle_text(cfg, seed, ids):
    _, t = specs(cfg)
    key = ("t", id(cfg), seed)
    if key not in _CACHE:
        _CACHE[key] = weights.text_weights(t, seed)
    return clip_ref.encode_text(_CACHE[key], t, ids)


def engine(cfg, tower, seed=1234, dtype="bf16", max_batch=64, **opts):
    """opts: open_clip_inference.engine.Engine's clipgpu_options keywords (gemm_tiles, lanes, graphs,
    prune_last, trim_text, ...)."""
    from open_clip_inference.engine import Engine
    return Engine(make_model_dir(cfg, seed), tower, [0], dtype, max_batch, **opts)


def check_rows(got, ref):
    cos = clip_ref.cosine_rows(got, ref)
    assert got.shape == ref.shape
    assert np.all(np.abs(np.linalg.norm(got, axis=1) - 1) < 1e-5)
    assert cos.min() >= COS_TOL, cos.min()
    return cos


@pytest.mark.parametrize("cfg,B", [(TINY_CFG, 3), (VIT_B_32_CFG, 4), (VIT_B_32_CFG, 5)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_vision_parity(cfg, B, dtype):
    v, _ = specs(cfg)
    u8 = weights.synth_images_u8(11 + B, B, v.image_size)
    px = normalized_pixels(u8, OPENAI_MEAN, OPENAI_STD)
    e = engine(cfg, 0, dtype=dtype)
    got = e.embed_pixels(px)
    check_rows(got, oracle_vision(cfg, 1234, px))


@pytest.mark.parametrize("cfg,B,random_eot", [(TINY_CFG, 5, True), (VIT_B_32_CFG, 6, False),
                                              (VIT_B_32_CFG, 7, True), (TINY_SIGLIP_CFG, 5, True),
                                              (TINY_SIGLIP_CFG, 3, False)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_text_parity(cfg, B, random_eot, dtype):
    _, t = specs(cfg)
    ids = weights.synth_token_ids(3 + B, B, t.context_length, t.vocab_size, t.vocab_size - 2,
                                  t.vocab_size - 1, random_eot=random_eot)
    e = engine(cfg, 1, dtype=dtype)
    got = e.embed_tokens(ids)
    check_rows(got, oracle_text(cfg, 1234, ids))


@pytest.mark.parametrize("residual,fold", [("f32", None), ("f16", False), ("f16", None)],
                         ids=["f32", "f16-ln-kernels", "f16-ln-folded"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_residual_stream_storage_parity(residual, fold, dtype):
    """clipgpu_options.residual / ln_fold (ABI v4): the residual stream stored in f32 or in f16 (every
    add and LayerNorm statistic in f32), with the LayerNorm kernels or with ln_1 / ln_2 folded into the
    QKV / c_fc GEMMs (the f16 default).  Both towers at ViT-B/32 dims against the fp64 oracle at the
    north-star bar, the lanes / pruning / trimming paths included (a batch over max_batch, host ids
    with random EOTs), and within 2e-5 of the f32 stream's cosine to the oracle."""
    v, t = specs(VIT_B_32_CFG)
    u8 = weights.synth_images_u8(41, 9, v.image_size)
    px = normalized_pixels(u8, OPENAI_MEAN, OPENAI_STD)
    ids = weights.synth_token_ids(41, 9, t.context_length, t.vocab_size, t.vocab_size - 2, t.vocab_size - 1,
                                  random_eot=True)
    ref_v, ref_t = oracle_vision(VIT_B_32_CFG, 1234, px), oracle_text(VIT_B_32_CFG, 1234, ids)
    cos = {}
    for res in ("f32", residual):
        fo = fold if res == residual else None
        ve = engine(VIT_B_32_CFG, 0, dtype=dtype, max_batch=8, residual=res, ln_fold=fo)
        te = engine(VIT_B_32_CFG, 1, dtype=dtype, max_batch=8, residual=res, ln_fold=fo)
        cos[res] = (check_rows(ve.embed_pixels(px), ref_v).min(), check_rows(te.embed_tokens(ids), ref_t).min())
        # the device-resident path (graphs, lanes) gives the same rows as the host path
        import torch
        d_px = torch.from_numpy(px[:8]).cuda()
        out = torch.empty((8, 512), device="cuda")
        ve.embed_pixels_device(d_px.data_ptr(), 8, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), ve.embed_pixels(px[:8]))
    assert cos[residual][0] >= cos["f32"][0] - 2e-5 and cos[residual][1] >= cos["f32"][1] - 2e-5, cos


def test_vision_u8_path_matches_f32_path():
    v, _ = specs(VIT_B_32_CFG)
    u8 = weights.synth_images_u8(21, 3, v.image_size)
    e = engine(VIT_B_32_CFG, 0)
    a = e.embed_u8(u8, OPENAI_MEAN, OPENAI_STD)
    b = e.embed_pixels(normalized_pixels(u8, OPENAI_MEAN, OPENAI_STD))
    # device-side normalize_pixels is bit-identical to the host one
    assert np.array_equal(a, b)


def test_vision_chunking_and_order():
    """B > max_batch is processed in chunks; rows stay in input order."""
    v, _ = specs(TINY_CFG)
    u8 = weights.synth_images_u8(5, 11, v.image_size)
    px = normalized_pixels(u8, OPENAI_MEAN, OPENAI_STD)
    e = engine(TINY_CFG, 0, max_batch=4)
    got = e.embed_pixels(px)
    check_rows(got, oracle_vision(TINY_CFG, 1234, px))
    single = np.concatenate([e.embed_pixels(px[i:i + 1]) for i in range(0, 11, 5)])
    assert np.allclose(single, got[0:11:5], atol=1e-6)


def test_text_pads_after_eot_do_not_matter():
    """Causal mask + argmax pooling: tokens after EOT cannot change the output (a18)."""
    _, t = specs(TINY_CFG)
    ids = weights.synth_token_ids(9, 4, t.context_length, t.vocab_size, t.vocab_size - 2, t.vocab_size - 1,
                                  random_eot=True)
    ids2 = ids.copy()
    for b in range(4):
        p = int(np.argmax(ids[b]))
        ids2[b, p + 1:] = (ids2[b, p + 1:] + 17) % (t.vocab_size - 2)
    e = engine(TINY_CFG, 1)
    assert np.array_equal(e.embed_tokens(ids), e.embed_tokens(ids2))


def test_errors():
    from open_clip_inference.error import InferenceError, ShapeError
    e = engine(TINY_CFG, 0)
    with pytest.raises(InferenceError, match="Empty batch"):
        e.embed_pixels(np.zeros((0, 3, 64, 64), np.float32))
    with pytest.raises(ShapeError):
        e.embed_pixels(np.zeros((1, 3, 32, 32), np.float32))
    t = engine(TINY_CFG, 1)
    with pytest.raises(InferenceError, match="out of range"):
        t.embed_tokens(np.full((1, 16), 5000, np.int64))


def test_device_entry_points():
    import torch  # device buffers only
    v, t = specs(TINY_CFG)
    u8 = weights.synth_images_u8(2, 3, v.image_size)
    px = normalized_pixels(u8, OPENAI_MEAN, OPENAI_STD)
    e = engine(TINY_CFG, 0)
    d_in = torch.from_numpy(px).cuda()
    d_out = torch.empty((3, v.embed_dim), device="cuda")
    s = torch.cuda.current_stream()
    e.embed_pixels_device(d_in.data_ptr(), 3, d_out.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    assert np.allclose(d_out.cpu().numpy(), e.embed_pixels(px), atol=1e-6)
    d_u8 = torch.from_numpy(u8).cuda()
    e.embed_u8_device(d_u8.data_ptr(), 3, OPENAI_MEAN, OPENAI_STD, d_out.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    assert np.allclose(d_out.cpu().numpy(), e.embed_pixels(px), atol=1e-6)
    ids = weights.synth_token_ids(1, 2, t.context_length, t.vocab_size, t.vocab_size - 2, t.vocab_size - 1)
    te = engine(TINY_CFG, 1)
    d_ids = torch.from_numpy(ids).cuda()
    d_o = torch.empty((2, t.embed_dim), device="cuda")
    te.embed_tokens_device(d_ids.data_ptr(), 2, d_o.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    assert np.allclose(d_o.cpu().numpy(), te.embed_tokens(ids), atol=1e-6)


@pytest.mark.parametrize("tower", [0, 1])
def test_graph_replay_reads_fresh_inputs_and_matches_direct_launches(tower):
    """Forwards replayed as hipGraphs (the default) are bit-identical to direct launches
    (clipgpu_options.graphs = -1), and a replay with the same buffers sees new input contents: device
    entry points (caller stream, fork/join) and host entry points (lane-slot streams)."""
    import torch
    v, t = specs(VIT_B_32_CFG)
    outs = {}
    for graphs in ["1", "0"]:
        e = engine(VIT_B_32_CFG, tower, max_batch=20, graphs=graphs == "1")
        res = []
        for seed in (51, 52, 53):
            if tower == 0:
                x = normalized_pixels(weights.synth_images_u8(seed, 20, v.image_size), OPENAI_MEAN, OPENAI_STD)
                host = e.embed_pixels(x)
            else:
                x = weights.synth_token_ids(seed, 20, t.context_length, t.vocab_size, t.vocab_size - 2,
                                            t.vocab_size - 1, random_eot=True)
                host = e.embed_tokens(x)
            if seed == 51:
                d_in = torch.from_numpy(x).cuda()
                d_out = torch.empty((20, 512), device="cuda")
            else:
                d_in.copy_(torch.from_numpy(x))
            s = torch.cuda.current_stream()
            if tower == 0:
                e.embed_pixels_device(d_in.data_ptr(), 20, d_out.data_ptr(), s.cuda_stream)
            else:
                e.embed_tokens_device(d_in.data_ptr(), 20, d_out.data_ptr(), s.cuda_stream)
            torch.cuda.synchronize()
            dev = d_out.cpu().numpy()
            assert np.array_equal(dev, host)
            res.append(host)
        outs[graphs] = res
    for a, b in zip(outs["1"], outs["0"]):
        assert np.array_equal(a, b)
    assert not np.array_equal(outs["1"][0], outs["1"][1])
    v0 = outs["1"][2][:3]
    if tower == 0:
        ref = oracle_vision(VIT_B_32_CFG, 1234, normalized_pixels(weights.synth_images_u8(53, 20, v.image_size),
                                                                  OPENAI_MEAN, OPENAI_STD)[:3])
    else:
        ref = oracle_text(VIT_B_32_CFG, 1234, weights.synth_token_ids(53, 20, t.context_length, t.vocab_size,
                                                                      t.vocab_size - 2, t.vocab_size - 1,
                                                                      random_eot=True)[:3])
    check_rows(v0, ref)


@pytest.mark.parametrize("tower,kind,mb", [(0, "u8", 20), (0, "u8", 40), (0, "f32", 40), (1, "ids", 20)])
def test_registered_host_buffers_are_bit_exact(tower, kind, mb):
    """Host entry points over caller-registered ranges (clipgpu_host_register: direct DMA) give the
    staged path's bytes: registered input, output or both; batches of 1, 5, a ragged 37 and 60
    (rounds of max_batch; with max_batch 40 vision cuts a round into the 5/32, 11/32, 16/32 chunks of
    host_chunks, proportionally for rounds of >= 20 rows), bit-equal across the two partitions.
    Overlapping registration is refused."""
    from open_clip_inference.engine import host_register, host_unregister
    from open_clip_inference.error import ClipError
    v, t = specs(VIT_B_32_CFG)
    # text: trimming off, so the ids are DMA'd from the registered range (a trimmed batch is a copy)
    e = engine(VIT_B_32_CFG, tower, max_batch=mb, lanes=2, **({"trim_text": False} if tower else {}))
    B = 60
    if kind == "u8":
        data = weights.synth_images_u8(61, B, v.image_size)
        run = lambda x, out: e.embed_u8(x, OPENAI_MEAN, OPENAI_STD, out=out)
    elif kind == "f32":
        data = normalized_pixels(weights.synth_images_u8(61, B, v.image_size), OPENAI_MEAN, OPENAI_STD)
        run = lambda x, out: e.embed_pixels(x, out=out)
    else:
        data = weights.synth_token_ids(61, B, t.context_length, t.vocab_size, t.vocab_size - 2,
                                       t.vocab_size - 1, random_eot=True)
        run = lambda x, out: e.embed_tokens(x, out=out)
    from open_clip_inference.engine import host_buffer
    buf = host_buffer(data.shape, data.dtype)
    buf[...] = data
    data = buf
    want = {n: run(data[:n], None) for n in (1, 5, 37, 60)}
    key = ("host_want", tower, kind)
    if key in _CACHE:  # the other max_batch's partition gave the same bytes
        assert all(np.array_equal(want[n], _CACHE[key][n]) for n in want)
    _CACHE[key] = want
    out = host_buffer((B, 512), np.float32)
    for reg_in, reg_out in [(1, 0), (0, 1), (1, 1)]:
        if reg_in:
            host_register(data)
        if reg_out:
            host_register(out)
        try:
            for n in (1, 5, 37, 60):
                out[:] = np.nan
                got = run(data[:n], out[:n])
                assert np.array_equal(got, want[n]), (reg_in, reg_out, n)
                assert np.isnan(out[n:]).all()
        finally:
            if reg_in:
                host_unregister(data)
            if reg_out:
                host_unregister(out)
    host_register(data)
    try:
        with pytest.raises(ClipError, match="overlaps"):
            host_register(data[1:])
    finally:
        host_unregister(data)
    # a range on a registered range's page that does not overlap it is refused too (registration pins
    # whole pages): 100 bytes registered, then 64 bytes 200 bytes further on the same page
    small = host_buffer((100,), np.uint8)
    host_register(small)
    try:
        same_page = np.frombuffer((ctypes.c_uint8 * 64).from_address(small.ctypes.data + 200), np.uint8)
        with pytest.raises(ClipError, match="shares a memory page"):
            host_register(same_page)
    finally:
        host_unregister(small)


def test_native_library_is_loaded():
    """The HIP library, not a fallback, is what ran (one libamdhip64 in-process)."""
    import re
    from open_clip_inference import _lib
    _lib.lib()
    maps = open("/proc/self/maps").read()
    assert "libclipgpu.so" in maps
    hip = set(re.findall(r"\S*libamdhip64\S*", maps))
    assert len(hip) == 1, hip


@pytest.mark.parametrize("tower", [0, 1])
def test_gemm_tile_choice_is_bit_exact(tower):
    """Every GEMM tile the library builds computes the same K-ordered sums: the tile table and the
    creation-time tuner change speed, never the embeddings."""
    from open_clip_inference import _lib
    v, t = specs(VIT_B_32_CFG)
    if tower == 0:
        data = normalized_pixels(weights.synth_images_u8(31, 48, v.image_size), OPENAI_MEAN, OPENAI_STD)
    else:
        data = weights.synth_token_ids(31, 48, t.context_length, t.vocab_size, t.vocab_size - 2,
                                       t.vocab_size - 1, random_eot=True)
    outs = []
    pins = [[t] * 4 for t in BUILT_TILES] + [[18, 26, 18, 26], [18, 17, 18, 17], [14, 15, 3, 26], None]
    for tiles in pins:
        e = engine(VIT_B_32_CFG, tower, max_batch=48, gemm_tiles=tiles, patch_tile=tiles[3] if tiles else 0)
        got = (c_int * 4)()
        _lib.check(_lib.lib().clipgpu_test_engine_tiles(e._h, got))
        if tiles:
            assert list(got) == tiles
        else:
            assert all(x == 0 or x in BUILT_TILES for x in got), list(got)
        outs.append(e.embed_pixels(data) if tower == 0 else e.embed_tokens(data))
    bad = [(pins[i], float(np.abs(o - outs[0]).max())) for i, o in enumerate(outs) if not np.array_equal(o, outs[0])]
    assert not bad, bad


@pytest.mark.parametrize("tower", [0, 1])
def test_chunked_gemm_launches_are_bit_exact(tower):
    """launch_gemm's row-chunked path (operands past 2^31 bytes: a ViT-L / H engine at max_batch ~1024)
    on a CLIP-family engine with the f16 residual stream and the LayerNorm fold (the defaults): with the
    chunk cap lowered to 256 rows (clipgpu_test_gemm_chunk_rows) every trunk GEMM, the patch GEMM
    included, runs as several launches; the embeddings are bit-equal to the unchunked engine's.  (ADVICE
    r5: the chunks used to address the f16 stream at f32 strides and reuse chunk 0's row statistics.)"""
    from open_clip_inference import _lib
    v, t = specs(VIT_B_32_CFG)
    if tower == 0:
        data = normalized_pixels(weights.synth_images_u8(57, 16, v.image_size), OPENAI_MEAN, OPENAI_STD)
    else:
        data = weights.synth_token_ids(57, 16, t.context_length, t.vocab_size, t.vocab_size - 2,
                                       t.vocab_size - 1, random_eot=True)
    run = (lambda e: e.embed_pixels(data)) if tower == 0 else (lambda e: e.embed_tokens(data))
    _lib.check(_lib.lib().clipgpu_test_gemm_chunk_rows(256))
    try:
        chunked = run(engine(VIT_B_32_CFG, tower, max_batch=16))
    finally:
        _lib.check(_lib.lib().clipgpu_test_gemm_chunk_rows(0))
    whole = run(engine(VIT_B_32_CFG, tower, max_batch=16))
    np.testing.assert_array_equal(chunked, whole)
    check_rows(whole[:3], oracle_vision(VIT_B_32_CFG, 1234, data[:3]) if tower == 0
               else oracle_text(VIT_B_32_CFG, 1234, data[:3]))


def test_removed_bt_tile_pin_is_refused():
    """Tile 1 (the 128x128 bt kernel, removed in round 6: run-to-run wrong outputs) is no
    longer a built tile: a pin of it fails at creation instead of running a kernel that is gone."""
    from open_clip_inference.error import ClipError
    with pytest.raises(ClipError):
        engine(TINY_CFG, 0, max_batch=4, gemm_tiles=[1, 1, 1, 1])


@pytest.mark.parametrize("tower", [0, 1])
def test_concurrent_lanes_are_bit_exact(tower):
    """Splitting a batch over concurrent lanes (sub-batches on their own streams)
    is invisible in the output: rows never interact outside attention."""
    v, t = specs(VIT_B_32_CFG)
    if tower == 0:
        data = normalized_pixels(weights.synth_images_u8(41, 37, v.image_size), OPENAI_MEAN, OPENAI_STD)
    else:
        data = weights.synth_token_ids(41, 37, t.context_length, t.vocab_size, t.vocab_size - 2,
                                       t.vocab_size - 1, random_eot=True)
    outs = []
    for lanes in [1, 2, 3, 4]:
        e = engine(VIT_B_32_CFG, tower, max_batch=37, gemm_tiles=[15, 15, 15, 15], lanes=lanes)
        outs.append(e.embed_pixels(data) if tower == 0 else e.embed_tokens(data))
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    ref = oracle_vision(VIT_B_32_CFG, 1234, data[:4]) if tower == 0 else oracle_text(VIT_B_32_CFG, 1234, data[:4])
    check_rows(outs[-1][:4], ref)


@pytest.mark.parametrize("cfg", [VIT_B_32_CFG, TINY_CFG, TINY_SIGLIP_CFG])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("tower", [0, 1])
def test_last_layer_pruning_is_bit_exact(cfg, dtype, tower):
    """The last layer run on the pooled rows only (CLS / EOT argmax gathered after attention,
    engine/forward.hip trunk) gives the same bits as the full last layer: every op after attention is
    row-local and each kept row goes through the same kernels.  Random EOT positions, two
    lanes, and a batch whose rows-per-lane exceed the token count (gather sources and
    destinations interleave)."""
    if dtype == "fp8" and cfg in (TINY_CFG, TINY_SIGLIP_CFG):
        pytest.skip("fp8 engines need MX-sized widths (multiples of 128)")
    if cfg is TINY_SIGLIP_CFG and tower == 0:
        pytest.skip("SigLIP vision pools every token (MAP head): no pruning")
    v, t = specs(cfg)
    B = 37
    if tower == 0:
        data = normalized_pixels(weights.synth_images_u8(43, B, v.image_size), OPENAI_MEAN, OPENAI_STD)
    else:
        data = weights.synth_token_ids(43, B, t.context_length, t.vocab_size, t.vocab_size - 2,
                                       t.vocab_size - 1, random_eot=True)
    outs = {}
    for prune in ["0", "1"]:
        e = engine(cfg, tower, dtype=dtype, max_batch=B, lanes=2, prune_last=prune == "1")
        outs[prune] = e.embed_pixels(data) if tower == 0 else e.embed_tokens(data)
        outs[prune + "s"] = e.embed_pixels(data[:3]) if tower == 0 else e.embed_tokens(data[:3])
    assert np.array_equal(outs["0"], outs["1"])
    assert np.array_equal(outs["0s"], outs["1s"])
    if dtype == "bf16":
        ref = oracle_vision(cfg, 1234, data[:4]) if tower == 0 else oracle_text(cfg, 1234, data[:4])
        check_rows(outs["1"][:4], ref)


def test_siglip2_text_is_not_trimmed_and_pools_the_last_position():
    """SigLIP2's text tower (no causal mask, pool_type "last") attends to and pools the final
    context position, padding included: host ids are never trimmed (the host entry point equals
    the device one), and a token after a sequence's EOT changes its embedding."""
    import torch
    _, t = specs(TINY_SIGLIP_CFG)
    ids = weights.synth_token_ids(77, 6, t.context_length, t.vocab_size, t.vocab_size - 2, t.vocab_size - 1,
                                  random_eot=True)
    e = engine(TINY_SIGLIP_CFG, 1, max_batch=8)
    host = e.embed_tokens(ids)
    d_in = torch.from_numpy(ids).cuda()
    d_out = torch.empty((6, e.embed_dim), device="cuda")
    e.embed_tokens_device(d_in.data_ptr(), 6, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), host)
    ids2 = ids.copy()
    p = int(np.argmax(ids2[0]))
    ids2[0, p + 1:] = 7
    other = e.embed_tokens(ids2)
    assert not np.array_equal(other[0], host[0]) and np.array_equal(other[1:], host[1:])
    check_rows(other, oracle_text(TINY_SIGLIP_CFG, 1234, ids2))


@pytest.mark.parametrize("cfg,max_eot", [(VIT_B_32_CFG, 9), (VIT_B_32_CFG, 30), (VIT_B_32_CFG, 76), (TINY_CFG, 5)])
def test_text_trim_is_bit_exact(cfg, max_eot):
    """Host-ids text batches run on their first max(EOT) + 1 tokens (at least 16;
    clipgpu_embed_tokens): causal attention keeps the tokens after a sequence's EOT away from
    its pooled row, so the embeddings equal the full-context run bit for bit.  Short captions
    (EOT at 2..max_eot, zero padding after), a batch over two lanes and several slots."""
    _, t = specs(cfg)
    B = 37
    rng = np.random.default_rng(max_eot)
    ids = np.zeros((B, t.context_length), np.int64)
    ids[:, 0] = t.vocab_size - 2
    eot = rng.integers(2, max_eot + 1, B)
    eot[0] = max_eot
    for b in range(B):
        ids[b, 1:eot[b]] = rng.integers(1, t.vocab_size - 3, eot[b] - 1)
        ids[b, eot[b]] = t.vocab_size - 1
    outs = {}
    for trim in ["0", "1"]:
        e = engine(cfg, 1, max_batch=16, trim_text=trim == "1")
        outs[trim] = e.embed_tokens(ids)
    assert np.array_equal(outs["0"], outs["1"])
    check_rows(outs["1"][:4], oracle_text(cfg, 1234, ids[:4]))


@pytest.mark.parametrize("external", [False, True])
def test_onnx_model_folder_matches_seeded_weights(tmp_path, external):
    """A model folder in the reference's own format (visual.onnx / text.onnx from a
    torch.onnx.export with pull_onnx.py's arguments) embeds bit-identically to the same
    weights given as seeds."""
    import json
    from open_clip_inference.engine import Engine
    from oracle.model_spec import OPENAI_MODEL_CONFIG
    from tests.onnx_export import export_model_dir
    d = tmp_path / "onnx"
    d.mkdir()
    with open(d / "open_clip_config.json", "w") as f:
        json.dump(TINY_CFG, f)
    with open(d / "model_config.json", "w") as f:
        json.dump(OPENAI_MODEL_CONFIG, f)
    v, t = specs(TINY_CFG)
    export_model_dir(str(d), v, t, seed=1234, external=external)
    px = normalized_pixels(weights.synth_images_u8(8, 5, v.image_size), OPENAI_MEAN, OPENAI_STD)
    ids = weights.synth_token_ids(8, 5, t.context_length, t.vocab_size, t.vocab_size - 2, t.vocab_size - 1,
                                  random_eot=True)
    for tower, data in ((0, px), (1, ids)):
        a = Engine(str(d), tower, [0], "bf16", 16)
        b = engine(TINY_CFG, tower, seed=1234, max_batch=16)
        ea = a.embed_pixels(data) if tower == 0 else a.embed_tokens(data)
        eb = b.embed_pixels(data) if tower == 0 else b.embed_tokens(data)
        assert np.array_equal(ea, eb)
        ref = oracle_vision(TINY_CFG, 1234, data) if tower == 0 else oracle_text(TINY_CFG, 1234, data)
        check_rows(ea, ref)


@pytest.mark.parametrize("cfg,B", [(TINY_H14_CFG, 3), (LONG_H14_CFG, 2)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_vit_h14_structure_parity(cfg, B, dtype):
    """ViT-H/14 structure (BASELINE configs[4]): patch 14 (K = 588 zero-padded to 640,
    element-wise patch gather), head dim 80, erf GELU, up to 290 tokens (tiled attention)."""
    v, t = specs(cfg)
    u8 = weights.synth_images_u8(41 + B, B, v.image_size)
    e = engine(cfg, 0, dtype=dtype)
    got = e.embed_pixels(normalized_pixels(u8, OPENAI_MEAN, OPENAI_STD))
    check_rows(got, oracle_vision(cfg, 1234, normalized_pixels(u8, OPENAI_MEAN, OPENAI_STD)))
    assert np.array_equal(got, e.embed_u8(u8, OPENAI_MEAN, OPENAI_STD))


def test_vit_h14_378_full_dims():
    """DFN5B-CLIP-ViT-H-14-378 at full size (32 x 1280, 730 tokens; text 24 x 1024) vs the fp64
    oracle on seeded weights."""
    v, t = specs(VIT_H_14_378_CFG)
    u8 = weights.synth_images_u8(3, 2, v.image_size)
    px = normalized_pixels(u8, OPENAI_MEAN, OPENAI_STD)
    e = engine(VIT_H_14_378_CFG, 0, max_batch=2)
    check_rows(e.embed_pixels(px), oracle_vision(VIT_H_14_378_CFG, 1234, px))
    ids = weights.synth_token_ids(4, 3, t.context_length, t.vocab_size, t.vocab_size - 2, t.vocab_size - 1,
                                  random_eot=True)
    te = engine(VIT_H_14_378_CFG, 1, max_batch=3)
    check_rows(te.embed_tokens(ids), oracle_text(VIT_H_14_378_CFG, 1234, ids))


@pytest.mark.parametrize("cfg,B", [(TINY_SIGLIP_CFG, 3), (LONG_SIGLIP_CFG, 2)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_siglip_structure_parity(cfg, B, dtype):
    """SigLIP family (BASELINE configs[3] structure): timm trunk names, patch-conv bias, no class
    token, head dim 72, MLP 1000 -> 1024 zero-padded, tanh-GELU, eps 1e-6, MAP head; up to 576 tokens."""
    v, _ = specs(cfg)
    u8 = weights.synth_images_u8(51 + B, B, v.image_size)
    px = normalized_pixels(u8, SIGLIP_MEAN, SIGLIP_STD)
    e = engine(cfg, 0, dtype=dtype)
    got = e.embed_pixels(px)
    check_rows(got, oracle_vision(cfg, 1234, px))
    assert np.array_equal(got, e.embed_u8(u8, SIGLIP_MEAN, SIGLIP_STD))


def test_so400m_siglip2_384_full_dims():
    """ViT-SO400M-16-SigLIP2-384 vision at full size (27 x 1152, 576 tokens, MLP 4304) vs the oracle."""
    v, _ = specs(SO400M_16_SIGLIP2_384_CFG)
    px = normalized_pixels(weights.synth_images_u8(7, 2, v.image_size), SIGLIP_MEAN, SIGLIP_STD)
    e = engine(SO400M_16_SIGLIP2_384_CFG, 0, max_batch=2)
    check_rows(e.embed_pixels(px), oracle_vision(SO400M_16_SIGLIP2_384_CFG, 1234, px))


def test_graph_cache_eviction_with_varied_caption_lengths():
    """More distinct forwards than the hipGraph cache holds (32): host-ids text batches of varied
    size and max-EOT position (trimmed lengths bucketed to multiples of 16) evict the least
    recently used graphs after draining every replica stream; every call still equals the
    untrimmed, graph-free run bit for bit, and the engine keeps working."""
    _, t = specs(VIT_B_32_CFG)
    rng = np.random.default_rng(2024)
    e = engine(VIT_B_32_CFG, 1, max_batch=24)
    ref_engine = engine(VIT_B_32_CFG, 1, max_batch=24, graphs=False, trim_text=False)
    for call in range(44):
        B = int(rng.integers(1, 25))
        max_eot = int(rng.integers(2, t.context_length))
        ids = np.zeros((B, t.context_length), np.int64)
        ids[:, 0] = t.vocab_size - 2
        eot = rng.integers(1, max_eot + 1, B)
        eot[0] = max_eot
        for b in range(B):
            ids[b, 1:eot[b]] = rng.integers(1, t.vocab_size - 3, eot[b] - 1)
            ids[b, eot[b]] = t.vocab_size - 1
        got = e.embed_tokens(ids)
        assert np.array_equal(got, ref_engine.embed_tokens(ids)), (call, B, max_eot)
    check_rows(got[:2], oracle_text(VIT_B_32_CFG, 1234, ids[:2]))


# Real CLIP / DFN checkpoints carry a few "massive" residual channels: values in the hundreds in every
# token, against O(1) elsewhere.  The seeded init has none, so these tests plant them: an offset on a
# few channels at the stream's start (vision: ln_pre's bias, whose output IS the stream; text: the
# token table), grown by every layer's c_proj bias, written as the model folder's safetensors file so
# that the engine and the fp64 oracle run the very same weights.
MASSIVE_CHANNELS = (5, 131, 402)
MASSIVE_START, MASSIVE_PER_LAYER = 300.0, 12.0


def _massive_weights(cfg, tower, seed=1234):
    v, t = specs(cfg)
    if tower == 0:
        w = {k: a.copy() for k, a in weights.vision_weights(v, seed).items()}
        w["visual.ln_pre.bias"][list(MASSIVE_CHANNELS)] += MASSIVE_START
        pre, layers = "visual.transformer.resblocks.", v.layers
    else:
        w = {k: a.copy() for k, a in weights.text_weights(t, seed).items()}
        w["token_embedding.weight"][:, list(MASSIVE_CHANNELS)] += MASSIVE_START
        pre, layers = "transformer.resblocks.", t.layers
    for i in range(layers):
        w[f"{pre}{i}.mlp.c_proj.bias"][list(MASSIVE_CHANNELS)] += MASSIVE_PER_LAYER
    return w


def _massive_dir(cfg, tower, w):
    import os
    from safetensors.numpy import save_file
    d = make_model_dir(cfg, 1234)
    save_file({k: np.ascontiguousarray(a, np.float32) for k, a in w.items()},
              os.path.join(d, "open_clip_model.safetensors"))
    return d


@pytest.mark.parametrize("cfg,tower,B", [(VIT_B_32_CFG, 0, 4), (VIT_B_32_CFG, 1, 5), (VIT_H_14_378_CFG, 0, 2),
                                         (VIT_H_14_378_CFG, 1, 3)],
                         ids=["b32-vision", "b32-text", "h14-378-vision", "h14-text"])
def test_massive_residual_channels_parity(cfg, tower, B):
    """The f16 residual stream + LayerNorm fold (the CLIP-family default, round 5) on real-like
    activations: three channels carry 300 + 12 per layer in every token (up to
    ~690 in ViT-H/14's 32 layers).  Both storages against the fp64 oracle at the north-star 0.9999,
    and the f16 default within 2e-5 of the f32 stream's cosine; the cosines are in DESIGN.md §3."""
    from open_clip_inference.engine import Engine
    v, t = specs(cfg)
    w = _massive_weights(cfg, tower)
    d = _massive_dir(cfg, tower, w)
    if tower == 0:
        data = normalized_pixels(weights.synth_images_u8(91, B, v.image_size), OPENAI_MEAN, OPENAI_STD)
        ref = clip_ref.encode_image(w, v, data)
    else:
        data = weights.synth_token_ids(91, B, t.context_length, t.vocab_size, t.vocab_size - 2, t.vocab_size - 1,
                                       random_eot=True)
        ref = clip_ref.encode_text(w, t, data)
    cos = {}
    for res in ("f32", "f16"):
        e = Engine(d, tower, [0], "bf16", B, residual=res)
        got = e.embed_pixels(data) if tower == 0 else e.embed_tokens(data)
        cos[res] = float(check_rows(got, ref).min())
        e.close()
    print(f"massive-channel cos {cfg is VIT_H_14_378_CFG and 'h14' or 'b32'} tower {tower}: {cos}")
    assert cos["f16"] >= cos["f32"] - 2e-5, cos
