#!/usr/bin/env python3
"""Throughput of the BASELINE.json large configs and of the host-buffer path (1 GPU).

Not the bench.py contract line: configs[3] / configs[4] are parity-test cases there.  Reported
here per GPU at the per-GPU share of the BASELINE batch (SO400M-16-SigLIP2-384 vision 1024 / 8 =
128 images, DFN5B ViT-H/14-378 vision + text 512 / 8 = 64), device-resident inputs, seeded
weights, plus ViT-B/32 through the HOST entry points (u8 / f32 host buffers, pinned staging,
H2D + D2H included: the PCIe-inclusive rate SURVEY.md §8d asks to report beside the device one).
Prints one JSON line per measurement.
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: torch before the native lib)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "clip-embedder-rs_amd"))

from open_clip_inference import _lib  # noqa: E402
from open_clip_inference.engine import Engine  # noqa: E402
from oracle.model_spec import (OPENAI_MODEL_CONFIG, SO400M_16_SIGLIP2_384_CFG, VIT_B_32_CFG,  # noqa: E402
                               VIT_H_14_378_CFG)

# so400m_text: SigLIP2 text tower, 64 tokens x 27 layers x 2 (4 D^2 + 2 D MLP) + attention + projection
GFLOP = {"so400m_vision": 518.9, "h14_vision": 1007.0, "h14_text": 47.1, "b32_vision": 8.818, "so400m_text": 53.1}


def model_dir(cfg):
    d = tempfile.mkdtemp(prefix="clipgpu_models_")
    for name, obj in (("open_clip_config.json", cfg), ("model_config.json", OPENAI_MODEL_CONFIG),
                      ("clipgpu_synthetic.json", {"seed": 7})):
        with open(os.path.join(d, name), "w") as f:
            json.dump(obj, f)
    return d


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def device_leg(name, cfg, tower, B, steps=6, warmup=2, dtype="bf16", mx_sites=None, lanes=0):
    d = model_dir(cfg)
    e = Engine(d, tower, [0], dtype, B, mx_sites=mx_sites, lanes=lanes)
    s = torch.cuda.current_stream()
    mc = cfg["model_cfg"]
    E = mc["embed_dim"]
    out = torch.empty((B, E), device="cuda")
    if tower == 0:
        S = mc["vision_cfg"]["image_size"]
        x = torch.randn((B, 3, S, S), device="cuda")
        fn = lambda: e.embed_pixels_device(x.data_ptr(), B, out.data_ptr(), s.cuda_stream)  # noqa: E731
    else:
        T, V = mc["text_cfg"]["context_length"], mc["text_cfg"]["vocab_size"]
        ids = torch.randint(0, V - 2, (B, T), device="cuda", dtype=torch.int64)
        ids[:, -1] = V - 1
        fn = lambda: e.embed_tokens_device(ids.data_ptr(), B, out.data_ptr(), s.cuda_stream)  # noqa: E731
    dt = timed(fn, steps, warmup)
    rate = B / dt
    gf = GFLOP[name.replace("_fp8", "").replace("_full", "")]
    print(json.dumps({"measure": name, "dtype": dtype, "mx_sites": mx_sites if dtype == "fp8" else None,
                      "lanes": e.info()[1],
                      "batch_per_gpu": B, "units_per_s": round(rate, 1),
                      "ms_per_step": round(dt * 1e3, 3), "model_tflops": round(rate * gf / 1e3, 1),
                      "frac_of_2500": round(rate * gf / 1e3 / 2500, 4), "input": "device-resident"}),
          flush=True)
    e.close()


def host_leg(B=256, steps=6, warmup=2):
    d = model_dir(VIT_B_32_CFG)
    e = Engine(d, 0, [0], "bf16", B)
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (B, 224, 224, 3), dtype=np.uint8)
    mean, std = VIT_B_32_CFG["preprocess_cfg"]["mean"], VIT_B_32_CFG["preprocess_cfg"]["std"]
    px = ((u8.astype(np.float32) / 255 - np.asarray(mean, np.float32)) / np.asarray(std, np.float32))
    px = np.ascontiguousarray(px.transpose(0, 3, 1, 2))
    for kind, fn in (("host_u8", lambda: e.embed_u8(u8, mean, std)), ("host_f32", lambda: e.embed_pixels(px))):
        dt = timed(fn, steps, warmup)
        print(json.dumps({"measure": "b32_vision_" + kind, "batch": B, "units_per_s": round(B / dt, 1),
                          "ms_per_step": round(dt * 1e3, 3),
                          "input": "host buffer (pinned staging + H2D/D2H inside the timing)"}), flush=True)
    e.close()


def captions_leg(B=1024, steps=6, warmup=2):
    """ViT-B/32 text from host token ids at caption lengths (EOT at 8..24, zero padding to
    77): sequence trimming (clipgpu_embed_tokens runs the batch on its first max(EOT)+1
    tokens) on vs off (Engine(trim_text=False)).  Host buffers: H2D/D2H inside the timing."""
    d = model_dir(VIT_B_32_CFG)
    rng = np.random.default_rng(0)
    V = 49408
    ids = np.zeros((B, 77), np.int64)
    ids[:, 0] = V - 2
    eot = rng.integers(8, 25, B)
    for b in range(B):
        ids[b, 1:eot[b]] = rng.integers(1, V - 3, eot[b] - 1)
        ids[b, eot[b]] = V - 1
    res = {}
    for trim in ("1", "0"):
        e = Engine(d, 1, [0], "bf16", B, trim_text=trim == "1")
        dt = timed(lambda: e.embed_tokens(ids), steps, warmup)
        res[trim] = e.embed_tokens(ids)
        print(json.dumps({"measure": "b32_text_captions_" + ("trimmed" if trim == "1" else "full77"), "batch": B,
                          "max_eot": int(eot.max()), "units_per_s": round(B / dt, 1),
                          "ms_per_step": round(dt * 1e3, 3),
                          "input": "host token ids (pinned staging + H2D/D2H inside the timing)"}), flush=True)
        e.close()
    print(json.dumps({"measure": "b32_text_captions_bit_equal", "value": bool(np.array_equal(res["1"], res["0"]))}),
          flush=True)


def photos_leg(B=256, H=480, W=640, steps=4, warmup=1):
    """Decoded 640x480 photos -> embeddings (a3-a7 + forward, BASELINE configs[1] model): the
    reference's CPU resize path restated (host C++ preprocess_batch thread pool + embed_pixels)
    against the GPU crop/resize path (clipgpu_embed_images_rgb8); outputs bit-identical."""
    from open_clip_inference.engine import preprocess_batch_rgb8
    d = model_dir(VIT_B_32_CFG)
    e = Engine(d, 0, [0], "bf16", B)
    rng = np.random.default_rng(1)
    ims = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    pc = VIT_B_32_CFG["preprocess_cfg"]
    legs = (("photos_host_resize", lambda: e.embed_pixels(preprocess_batch_rgb8(ims, 224, "bicubic", "shortest",
                                                                                 pc["mean"], pc["std"]))),
            ("photos_gpu_resize", lambda: e.embed_images_rgb8(ims)))
    for kind, fn in legs:
        dt = timed(fn, steps, warmup)
        print(json.dumps({"measure": "b32_vision_" + kind, "batch": B, "image": f"{W}x{H} RGB8 (bicubic, shortest)",
                          "units_per_s": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 3),
                          "host_threads": min(16, os.cpu_count() or 1)}), flush=True)
    e.close()


def similarity_leg(ni=65536, nt=1000, E=512, steps=5, warmup=2):
    """Facade math on the device: [ni x E] images x [nt x E] labels -> softmax over labels
    (classify for a whole image set), device-resident embeddings; exact-f32 MFMA."""
    import ctypes
    a = torch.nn.functional.normalize(torch.randn(ni, E, device="cuda"), dim=1)
    b = torch.nn.functional.normalize(torch.randn(nt, E, device="cuda"), dim=1)
    out = torch.empty(ni, nt, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L = _lib.lib()

    def run():
        _lib.check(L.clipgpu_similarity_device(ctypes.c_void_p(a.data_ptr()), ni, ctypes.c_void_p(b.data_ptr()), nt, E,
                                               100.0, 0.0, 0, 1, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s)))
    dt = timed(run, steps, warmup)
    ref = torch.softmax(100.0 * a @ b.T, dim=1)
    err = float((out - ref).abs().max())
    print(json.dumps({"measure": "similarity_softmax", "n_img": ni, "n_txt": nt, "E": E,
                      "ms": round(dt * 1e3, 3), "tflops_f32": round(2 * ni * nt * E / dt / 1e12, 1),
                      "max_abs_err_vs_torch": err}), flush=True)


INDEX_DTYPES = {"f32": (4, None), "f16": (2, torch.float16), "bf16": (2, torch.bfloat16)}


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(v, nbytes):
    med = float(np.median(v))
    return {"ms_median": round(med, 3), "ms_min_max": [round(min(v), 3), round(max(v), 3)],
            "gallery_TBps": round(nbytes / (med * 1e-3) / 1e12, 2)}


def topk_leg(N=1 << 20, E=512, k=10, runs=7, warmup=2, Qs=(1, 4, 16, 17, 32, 256), dtypes=("f32", "f16", "bf16")):
    """Semantic search over a device-resident gallery of N embeddings, per query count and index storage
    type: three legs alternate in one process -- the fused search on its default route
    (clipgpu_index_search_device: the few-query kernel up to kNarrowRows query rows), the fused search
    forced onto the wide kernel (clipgpu_test_topk_route 1: the only kernel before the few-query one
    existed), and the same result by the full-matrix path (clipgpu_similarity_device logits into a
    [Q][N] tensor, then torch.topk), which for a 16-bit index runs on the widened rounded gallery.  Per
    leg the median and the spread of `runs` device-event timings after `warmup` rounds (the order of
    the legs rotates from round to round: what a leg finds in the caches depends on the leg before it), and the
    effective gallery bandwidth N E elem / t; the floor beside them is one read of the gallery at
    6.3 TB/s.  All three legs return the same indices and bit-equal scores.  For the 16-bit types the
    line also carries the top-k overlap with the F32 index (a Gaussian gallery, not embedding data)."""
    import ctypes
    from open_clip_inference import EmbeddingIndex
    torch.manual_seed(0)
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.nn.functional.normalize(torch.randn(N, E, device="cuda"), dim=1)
    qs = {Q: torch.nn.functional.normalize(torch.randn(Q, E, device="cuda"), dim=1) for Q in Qs}
    f32_idx = {}
    try:
        for dt in dtypes:
            esz, tdt = INDEX_DTYPES[dt]
            gw = g if tdt is None else g.to(tdt).float()  # what the index holds, widened
            ix = EmbeddingIndex(E, N, dtype=dt)
            ix.add_device(g.data_ptr(), N, s)
            for Q in Qs:
                q = qs[Q]
                mat = torch.empty(Q, N, device="cuda")
                res = {name: (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), device="cuda"))
                       for name in ("default", "wide")}
                base = {}

                def fused(name, route):
                    _lib.check(L.clipgpu_test_topk_route(route))
                    ix.search_device(q.data_ptr(), Q, k, res[name][0].data_ptr(), res[name][1].data_ptr(), 100.0, 0.0, s)

                def baseline():
                    _lib.check(L.clipgpu_similarity_device(ctypes.c_void_p(q.data_ptr()), Q, ctypes.c_void_p(gw.data_ptr()),
                                                           N, E, 100.0, 0.0, 2, 1, ctypes.c_void_p(mat.data_ptr()),
                                                           ctypes.c_void_p(s)))
                    base["score"], base["idx"] = torch.topk(mat, k, dim=1)

                legs = (("default", lambda: fused("default", 0)), ("wide", lambda: fused("wide", 1)), ("baseline", baseline))
                ms = {name: [] for name, _ in legs}
                for rnd in range(warmup + runs):
                    for name, fn in legs[rnd % 3:] + legs[:rnd % 3]:  # every leg follows every other equally often
                        t = _event_ms(fn)
                        if rnd >= warmup:
                            ms[name].append(t)
                # the same result: scores bit for bit; indices once the baseline's ties are put in index order
                b_idx, b_score = base["idx"].cpu().numpy(), base["score"].cpu().numpy()
                order = np.lexsort((b_idx, -b_score.astype(np.float64)), axis=1)
                b_idx, b_score = np.take_along_axis(b_idx, order, 1), np.take_along_axis(b_score, order, 1)
                for name in ("default", "wide"):
                    assert np.array_equal(res[name][1].cpu().numpy().view(np.uint32), b_score.view(np.uint32)), name
                    assert np.array_equal(res[name][0].cpu().numpy(), b_idx), name
                nbytes = N * E * esz
                out = {"measure": "topk_search", "Q": Q, "dtype": dt, "N": N, "E": E, "k": k, "runs": runs,
                       "same_indices": True, "gallery_read_floor_ms_at_6.3TBps": round(nbytes / 6.3e12 * 1e3, 3),
                       "mfma_floor_ms_wide": round(2.0 * max(Q, 64) * N * E / 157.3e12 * 1e3, 3)}
                for name, v in ms.items():
                    out[name] = _stats(v, nbytes)
                out["default_over_wide"] = round(out["default"]["ms_median"] / out["wide"]["ms_median"], 3)
                out["default_over_baseline"] = round(out["default"]["ms_median"] / out["baseline"]["ms_median"], 3)
                if dt == "f32":
                    f32_idx[Q] = b_idx
                elif Q in f32_idx:
                    both = [len(set(a) & set(b)) for a, b in zip(b_idx.tolist(), f32_idx[Q].tolist())]
                    out["topk_overlap_with_f32"] = round(float(np.mean(both)) / k, 4)
                print(json.dumps(out), flush=True)
            ix.close()
    finally:
        _lib.check(L.clipgpu_test_topk_route(0))


def topk_range_leg(N=1 << 20, E=512, k=10, runs=7, warmup=2, Qs=(1, 16, 256), dtypes=("f32", "f16"), NJ=1 << 17,
                   min_cosine=0.2):
    """The range search against the search it shares its hot loop with, per query count and storage type:
    legs alternating in one process (rotating order, device-event timings after `warmup` rounds) --
    range_search_device at a threshold that about k rows per query pass (the median over the queries of the
    k-th score of a search), search_device(k) on the same inputs (the yardstick), and at Q = 16 also
    range_search_device at threshold -inf into a small buffer: every column a hit, the cost of dense
    emission (one counter add per wave and tile; nearly every record is dropped at the capacity).  The
    range leg's total is checked against the scores of a k = 128 search.  Then the self-join of NJ rows
    (EmbeddingIndex.duplicates at `min_cosine`, host form: launches, copy-back and host sort included, wall
    clock) against what a user does today, search_device of every row with k = 128 (wall clock to the end
    of the device work, without reading the result back or pairing it up)."""
    from open_clip_inference import EmbeddingIndex
    torch.manual_seed(0)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.nn.functional.normalize(torch.randn(N, E, device="cuda"), dim=1)
    qs = {Q: torch.nn.functional.normalize(torch.randn(Q, E, device="cuda"), dim=1) for Q in Qs}
    for dt in dtypes:
        esz, _ = INDEX_DTYPES[dt]
        with EmbeddingIndex(E, N, dtype=dt) as ix:
            ix.add_device(g.data_ptr(), N, s)
            for Q in Qs:
                q = qs[Q]
                idx128 = torch.empty((Q, 128), dtype=torch.int64, device="cuda")
                sc128 = torch.empty((Q, 128), device="cuda")
                ix.search_device(q.data_ptr(), Q, 128, idx128.data_ptr(), sc128.data_ptr(), 100.0, 0.0, s)
                thr = float(sc128[:, k - 1].median())
                expect = int((sc128 >= thr).sum())
                assert int((sc128[:, -1] >= thr).sum()) == 0  # 128 were enough to count the hits
                cap = 64 * Q + 1024
                rec = (torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"),
                       torch.empty(cap, device="cuda"))
                tot = {name: torch.zeros(1, dtype=torch.int64, device="cuda") for name in ("range", "dense")}
                idx, sc = torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), device="cuda")

                def ranged(name, t):
                    ix.range_search_device(q.data_ptr(), Q, t, cap, rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(),
                                           tot[name].data_ptr(), 100.0, 0.0, s)

                legs = [("range", lambda: ranged("range", thr)),
                        ("search", lambda: ix.search_device(q.data_ptr(), Q, k, idx.data_ptr(), sc.data_ptr(), 100.0, 0.0, s))]
                if Q == 16:
                    legs.append(("dense", lambda: ranged("dense", float("-inf"))))
                ms = {name: [] for name, _ in legs}
                for rnd in range(warmup + runs):
                    r = rnd % len(legs)
                    for name, fn in legs[r:] + legs[:r]:  # every leg follows every other equally often
                        t = _event_ms(fn)
                        if rnd >= warmup:
                            ms[name].append(t)
                assert int(tot["range"]) == expect, (int(tot["range"]), expect)
                nbytes = N * E * esz
                out = {"measure": "topk_range", "Q": Q, "dtype": dt, "N": N, "E": E, "k": k, "runs": runs,
                       "threshold": round(thr, 4), "hits": expect, "same_count_as_search": True}
                for name, v in ms.items():
                    out[name] = _stats(v, nbytes)
                out["range_over_search"] = round(out["range"]["ms_median"] / out["search"]["ms_median"], 3)
                if Q == 16:
                    assert int(tot["dense"]) == Q * N
                    out["dense_hits"], out["dense_capacity"] = Q * N, cap
                print(json.dumps(out), flush=True)
    # the self-join: NJ rows of the same gallery, f32
    gj = g[:NJ].contiguous()
    with EmbeddingIndex(E, NJ) as ix:
        ix.add_device(gj.data_ptr(), NJ, s)
        idx128 = torch.empty((NJ, 128), dtype=torch.int64, device="cuda")
        sc128 = torch.empty((NJ, 128), device="cuda")
        found = {}

        def join():
            found["pairs"], found["cos"] = ix.duplicates(min_cosine, max_pairs=1 << 22)

        def every_row():
            ix.search_device(gj.data_ptr(), NJ, 128, idx128.data_ptr(), sc128.data_ptr(), 1.0, 0.0, s)
            torch.cuda.synchronize()

        ms = {"self_join": [], "search_every_row_k128": []}
        for rnd in range(warmup + runs):
            for name, fn in (("self_join", join), ("search_every_row_k128", every_row)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if rnd >= warmup:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        # the same pairs: every result of the k = 128 searches above the cut, j > i, is a pair of the join
        hit = (sc128 >= min_cosine) & (idx128 > torch.arange(NJ, device="cuda")[:, None])
        assert int((sc128[:, -1] >= min_cosine).sum()) == 0 and int(hit.sum()) == len(found["pairs"])
        out = {"measure": "self_join", "N": NJ, "E": E, "dtype": "f32", "min_cosine": min_cosine, "runs": runs,
               "pairs": len(found["pairs"]), "same_pairs_as_search": True}
        for name, v in ms.items():
            med = float(np.median(v))
            out[name] = {"ms_median": round(med, 2), "ms_min_max": [round(min(v), 2), round(max(v), 2)]}
        med = out["self_join"]["ms_median"]
        out["tflops_f32_of_N2E"] = round(2.0 * NJ * NJ * E / (med * 1e-3) / 1e12, 1)  # the full square's FLOP / time
        out["derived_ms_at_N_2^20"] = round(med * (float(1 << 20) / NJ) ** 2, 0)
        print(json.dumps(out), flush=True)


def kmeans_leg(N=1 << 20, E=512, runs=7, warmup=2, Cs=(64, 1024), dtypes=("f32", "f16")):
    """One k-means iteration over a device-resident gallery, per centroid count and storage type, in its two
    halves and against what a user can do without them; legs alternating in one process (rotating order,
    device-event timings after `warmup` rounds):
      assign       clipgpu_index_assign_device, every row's nearest of C centroids;
      range        the yardstick: range_search_device of the same gallery with the C centroids as queries at a
                   threshold nothing passes -- the same FLOPs through the same tile loop;
      update       one update alone (clipgpu_test_index_kmeans_update: zero the sums, 64-bit integer atomic adds,
                   finalise);
      search_k1    the assignment today: search_device with k = 1 of every gallery row (widened to f32) against
                   an index of the centroids;
      index_add    the sums today: torch index_add_ of the widened rows into an f32 [C][E] tensor (float atomics;
                   without the normalisation).
    assign's labels and scores are checked against search_k1's, bit for bit.  The line also carries the wall
    clock of a whole EmbeddingIndex.kmeans of 3 iterations from host centroids (copies included)."""
    from open_clip_inference import EmbeddingIndex
    torch.manual_seed(0)
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.nn.functional.normalize(torch.randn(N, E, device="cuda"), dim=1)
    for dt in dtypes:
        esz, tdt = INDEX_DTYPES[dt]
        gw = g if tdt is None else g.to(tdt).float()  # what the index holds, widened
        with EmbeddingIndex(E, N, dtype=dt) as ix:
            ix.add_device(g.data_ptr(), N, s)
            for C in Cs:
                cen = gw[torch.randperm(N, device="cuda")[:C]].contiguous()
                new_cen = cen.clone()
                lab, sc = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, device="cuda")
                idx1, sc1 = torch.empty((N, 1), dtype=torch.int64, device="cuda"), torch.empty((N, 1), device="cuda")
                rec = (torch.empty(1024, dtype=torch.int32, device="cuda"), torch.empty(1024, dtype=torch.int32, device="cuda"),
                       torch.empty(1024, device="cuda"))
                tot = torch.zeros(1, dtype=torch.int64, device="cuda")
                sums = torch.zeros((C, E), device="cuda")
                shift = 62 - 1 - int(N).bit_length()  # unit rows: m <= 1
                with EmbeddingIndex(E, C) as cix:
                    cix.add_device(cen.data_ptr(), C, s)
                    ix.assign_device(cen.data_ptr(), C, lab.data_ptr(), sc.data_ptr(), 1.0, 0.0, s)
                    torch.cuda.synchronize()
                    lab64 = lab.long()

                    def update():
                        _lib.check(L.clipgpu_test_index_kmeans_update(ix.handle, lab.data_ptr(), C, shift, new_cen.data_ptr(), s))

                    def index_add():
                        sums.zero_()
                        sums.index_add_(0, lab64, gw)

                    legs = [("assign", lambda: ix.assign_device(cen.data_ptr(), C, lab.data_ptr(), sc.data_ptr(), 1.0, 0.0, s)),
                            ("range", lambda: ix.range_search_device(cen.data_ptr(), C, 1e30, 1024, rec[0].data_ptr(),
                                                                     rec[1].data_ptr(), rec[2].data_ptr(), tot.data_ptr(),
                                                                     1.0, 0.0, s)),
                            ("update", update),
                            ("search_k1", lambda: cix.search_device(gw.data_ptr(), N, 1, idx1.data_ptr(), sc1.data_ptr(),
                                                                    1.0, 0.0, s)),
                            ("index_add", index_add)]
                    ms = {name: [] for name, _ in legs}
                    for rnd in range(warmup + runs):
                        r = rnd % len(legs)
                        for name, fn in legs[r:] + legs[:r]:  # every leg follows every other equally often
                            t = _event_ms(fn)
                            if rnd >= warmup:
                                ms[name].append(t)
                    assert int(tot) == 0
                    assert torch.equal(lab.long(), idx1[:, 0]) and torch.equal(sc.view(torch.int32), sc1[:, 0].view(torch.int32))
                    # the update against the float sums of the baseline, loosely: the same centroids
                    ref = torch.nn.functional.normalize(sums.double(), dim=1).float()
                    err = float((new_cen - ref).abs().max())
                    assert err < 1e-5, err
                host_cen = cen.cpu().numpy()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                km = ix.kmeans(init=host_cen, max_iter=3)
                wall = (time.perf_counter() - t0) * 1e3
                out = {"measure": "kmeans", "C": C, "dtype": dt, "N": N, "E": E, "runs": runs, "shift": shift,
                       "same_labels_as_search_k1": True, "update_max_abs_diff_vs_float_sums": err,
                       "kmeans_3_iters_wall_ms": round(wall, 1), "kmeans_moved": km.moved.tolist()}
                for name, v in ms.items():
                    out[name] = _stats(v, N * E * esz)
                m = {name: out[name]["ms_median"] for name in ms}
                out["assign_over_range"] = round(m["assign"] / m["range"], 3)
                out["assign_over_search_k1"] = round(m["assign"] / m["search_k1"], 3)
                out["update_over_assign"] = round(m["update"] / m["assign"], 3)
                out["update_over_index_add"] = round(m["update"] / m["index_add"], 3)
                out["update_atomics_per_us"] = round(N * E / (m["update"] * 1e3), 0)
                print(json.dumps(out), flush=True)


def ivf_leg(N=1 << 20, E=512, k=10, runs=7, warmup=2, Cs=(256, 1024, 4096), nprobes=(1, 8, 32), Qs=(1, 16, 256),
            dtypes=("f32", "f16"), centres=1024, sigma=0.05):
    """The probed (IVF) search against the plain search, per storage type, list count, query count and nprobe.
    The gallery is CLUSTERED: unit rows around `centres` random centres (centre + sigma * Gaussian noise per
    element); the queries are fresh draws of the same mixture.  The Gaussian gallery of the other legs has
    nothing to partition.  Per (dtype, C): partition_kmeans (5 iterations) and then, per Q, legs alternating in one
    process (rotating order, device-event timings after `warmup` rounds): search_device -- unchanged code, the
    yardstick measured in the same process -- and search_probed_device at each nprobe.  Beside each probed leg:
    the rows read as a fraction of the gallery (the probed lists' lengths, mean over the queries) and recall@k
    against the plain search (a property of the data, reported, not a bar).  One-off costs: the wall clock of
    partition (assign + list build, synchronous) and of assign_device alone (device events); their difference
    is the build.  The one timing condition: at Q = 1, C = 1024, nprobe = 8, f32 the probed [min, max] lies
    wholly below the plain [min, max]; asserted after the lines are printed."""
    from open_clip_inference import EmbeddingIndex
    torch.manual_seed(0)
    s = torch.cuda.current_stream().cuda_stream
    cen0 = torch.nn.functional.normalize(torch.randn(centres, E, device="cuda"), dim=1)

    def draw(n):
        return torch.nn.functional.normalize(cen0[torch.randint(0, centres, (n,), device="cuda")] +
                                             sigma * torch.randn(n, E, device="cuda"), dim=1).contiguous()

    g = draw(N)
    qs = {Q: draw(Q) for Q in Qs}
    verdict = None
    for dt in dtypes:
        esz, _ = INDEX_DTYPES[dt]
        with EmbeddingIndex(E, N, dtype=dt) as ix:
            ix.add_device(g.data_ptr(), N, s)
            torch.cuda.synchronize()
            for C in Cs:
                t0 = time.perf_counter()
                km = ix.partition_kmeans(C, max_iter=5, seed=0)
                km_wall = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                counts = ix.partition(km.centroids)
                part_wall = (time.perf_counter() - t0) * 1e3
                dc = torch.from_numpy(km.centroids).cuda()
                lab, sc = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, device="cuda")
                assign_ms = [_event_ms(lambda: ix.assign_device(dc.data_ptr(), C, lab.data_ptr(), sc.data_ptr(), 1.0, 0.0, s))
                             for _ in range(3)]
                lens = torch.from_numpy(counts).cuda()
                print(json.dumps({"measure": "ivf_partition", "dtype": dt, "N": N, "E": E, "C": C,
                                  "partition_kmeans_5_iters_wall_ms": round(km_wall, 1),
                                  "partition_wall_ms": round(part_wall, 2), "assign_device_ms": round(min(assign_ms), 2),
                                  "build_ms_by_difference": round(part_wall - min(assign_ms), 2),
                                  "longest_list": int(counts.max()), "empty_lists": int((counts == 0).sum())}), flush=True)
                for Q in Qs:
                    q = qs[Q]
                    names = ["plain"] + [f"nprobe{p}" for p in nprobes]
                    res = {n: (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), device="cuda"))
                           for n in names}
                    prb = {p: torch.empty((Q, p), dtype=torch.int64, device="cuda") for p in nprobes}

                    def plain():
                        ix.search_device(q.data_ptr(), Q, k, res["plain"][0].data_ptr(), res["plain"][1].data_ptr(), 100.0, 0.0, s)

                    def probed(p):
                        n = f"nprobe{p}"
                        return lambda: ix.search_probed_device(q.data_ptr(), Q, k, p, res[n][0].data_ptr(), res[n][1].data_ptr(),
                                                               100.0, 0.0, s, 0, prb[p].data_ptr())

                    legs = [("plain", plain)] + [(f"nprobe{p}", probed(p)) for p in nprobes]
                    ms = {n: [] for n in names}
                    for rnd in range(warmup + runs):
                        r = rnd % len(legs)
                        for name, fn in legs[r:] + legs[:r]:  # every leg follows every other equally often
                            t = _event_ms(fn)
                            if rnd >= warmup:
                                ms[name].append(t)
                    want = res["plain"][0].cpu().numpy()
                    out = {"measure": "ivf_search", "dtype": dt, "N": N, "E": E, "C": C, "Q": Q, "k": k, "runs": runs,
                           "plain": _stats(ms["plain"], N * E * esz)}
                    for p in nprobes:
                        n = f"nprobe{p}"
                        got = res[n][0].cpu().numpy()
                        recall = float(np.mean([len(set(a) & set(b)) for a, b in zip(got.tolist(), want.tolist())])) / k
                        frac = float(lens[prb[p].clamp(min=0)].sum(dim=1).double().mean()) / N
                        st = _stats(ms[n], N * E * esz)
                        del st["gallery_TBps"]
                        st.update({"rows_read_fraction": round(frac, 5), f"recall_at_{k}": round(recall, 4),
                                   "plain_over_probed": round(out["plain"]["ms_median"] / st["ms_median"], 2)})
                        out[n] = st
                    print(json.dumps(out), flush=True)
                    if dt == "f32" and C == 1024 and Q == 1 and 8 in nprobes:
                        verdict = (max(ms["nprobe8"]), min(ms["plain"]))
    if verdict is not None:
        assert verdict[0] < verdict[1], f"probed max {verdict[0]} ms is not below plain min {verdict[1]} ms"


def codes_leg(N=1 << 20, E=512, k=10, runs=7, warmup=2, Qs=(1, 16, 256), refines=(32, 128), centres=1024, sigma=0.05):
    """The coded search (int8 coarse scan + exact re-rank) against the plain search on the ivf leg's clustered f32
    gallery.  Per Q, legs alternating in one process (rotating order, device-event timings after `warmup` rounds):
    search_device -- unchanged code, the yardstick measured in the same process -- and per refine
    search_coded_device whole, its coarse stage alone (the queries' codes, the scan, the candidates' merge) and its
    re-rank alone (clipgpu_test_codes_stage 1 and 2; the re-rank runs on the candidates the coarse leg before it
    left).  Beside each: recall@k against the plain search (a property of the data, reported, not a bar).  One-off:
    the time of enable_codes (wall clock, synchronised; allocation + coding 2^20 rows).  The one timing condition:
    at Q = 256, refine = 128 the coded [min, max] lies wholly below the plain [min, max]; asserted after the lines
    are printed."""
    from open_clip_inference import EmbeddingIndex, _lib
    torch.manual_seed(0)
    s = torch.cuda.current_stream().cuda_stream
    cen0 = torch.nn.functional.normalize(torch.randn(centres, E, device="cuda"), dim=1)

    def draw(n):
        return torch.nn.functional.normalize(cen0[torch.randint(0, centres, (n,), device="cuda")] +
                                             sigma * torch.randn(n, E, device="cuda"), dim=1).contiguous()

    def stage(v):
        _lib.check(_lib.lib().clipgpu_test_codes_stage(v))

    g = draw(N)
    qs = {Q: draw(Q) for Q in Qs}
    verdict = None
    with EmbeddingIndex(E, N) as ix:
        ix.add_device(g.data_ptr(), N, s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.enable_codes()
        ix.codes(0, 1)  # waits for the coding
        print(json.dumps({"measure": "codes_enable", "N": N, "E": E, "enable_codes_wall_ms": round((time.perf_counter() - t0) * 1e3, 2),
                          "codes_bytes": N * (E + 4)}), flush=True)
        for Q in Qs:
            q = qs[Q]
            names = ["plain"] + [f"{w}{r}" for r in refines for w in ("coded", "coarse", "rerank")]
            res = {n: (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), device="cuda"))
                   for n in names}

            def plain():
                ix.search_device(q.data_ptr(), Q, k, res["plain"][0].data_ptr(), res["plain"][1].data_ptr(), 100.0, 0.0, s)

            def coded(name, r, st):
                def fn():
                    stage(st)
                    try:
                        ix.search_coded_device(q.data_ptr(), Q, k, res[name][0].data_ptr(), res[name][1].data_ptr(), r,
                                               100.0, 0.0, s)
                    finally:
                        stage(0)
                return fn

            # the three legs of a refine stay together and in this order: the re-rank needs the coarse leg's candidates
            groups = [[("plain", plain)]] + [[(f"coded{r}", coded(f"coded{r}", r, 0)), (f"coarse{r}", coded(f"coarse{r}", r, 1)),
                                              (f"rerank{r}", coded(f"rerank{r}", r, 2))] for r in refines]
            ms = {n: [] for n in names}
            for rnd in range(warmup + runs):
                r0 = rnd % len(groups)
                for grp in groups[r0:] + groups[:r0]:
                    for name, fn in grp:
                        t = _event_ms(fn)
                        if rnd >= warmup:
                            ms[name].append(t)
            want = res["plain"][0].cpu().numpy()
            out = {"measure": "codes_search", "N": N, "E": E, "Q": Q, "k": k, "runs": runs, "plain": _stats(ms["plain"], N * E * 4)}
            for r in refines:
                got = res[f"coded{r}"][0].cpu().numpy()
                recall = float(np.mean([len(set(a) & set(b)) for a, b in zip(got.tolist(), want.tolist())])) / k
                st = _stats(ms[f"coded{r}"], N * (E + 4))
                st["codes_TBps"] = st.pop("gallery_TBps")
                for w in ("coarse", "rerank"):
                    v = ms[f"{w}{r}"]
                    st[w] = {"ms_median": round(float(np.median(v)), 3), "ms_min_max": [round(min(v), 3), round(max(v), 3)]}
                st.update({f"recall_at_{k}": round(recall, 4), "plain_over_coded": round(out["plain"]["ms_median"] / st["ms_median"], 2)})
                out[f"refine{r}"] = st
            print(json.dumps(out), flush=True)
            if Q == 256 and 128 in refines:
                verdict = (max(ms["coded128"]), min(ms["plain"]))
    if verdict is not None:
        assert verdict[0] < verdict[1], f"coded max {verdict[0]} ms is not below plain min {verdict[1]} ms"


def topk_routes_leg(N=1 << 20, E=512, k=10, runs=7, warmup=2, Qs=(1, 2, 4, 8, 12, 16)):
    """The measurement kNarrowRows (csrc/kernels/kernels.hpp) is set by: for every query count the
    few-query kernel can take, that kernel (route 2) against the wide one (route 1) on an f32 gallery,
    alternating in one process in a fixed order (each leg always follows the other; swapping the order
    from round to round would run a leg right after itself, on a gallery tail still in the cache, and
    measured 0.675 instead of 0.76 ms at Q = 16); kNarrowRows is the largest Q at which the few-query
    median is lower."""
    from open_clip_inference import EmbeddingIndex
    torch.manual_seed(0)
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.nn.functional.normalize(torch.randn(N, E, device="cuda"), dim=1)
    ix = EmbeddingIndex(E, N)
    ix.add_device(g.data_ptr(), N, s)
    try:
        for Q in Qs:
            q = torch.nn.functional.normalize(torch.randn(Q, E, device="cuda"), dim=1)
            res = {r: (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), device="cuda"))
                   for r in (1, 2)}

            def run(r):
                _lib.check(L.clipgpu_test_topk_route(r))
                ix.search_device(q.data_ptr(), Q, k, res[r][0].data_ptr(), res[r][1].data_ptr(), 100.0, 0.0, s)

            ms = {1: [], 2: []}
            for rnd in range(warmup + runs):
                for r in (2, 1):  # a fixed order: with two legs a swapped order makes a leg follow itself
                    t = _event_ms(lambda: run(r))
                    if rnd >= warmup:
                        ms[r].append(t)
            assert torch.equal(res[1][0], res[2][0]) and torch.equal(res[1][1].view(torch.int32), res[2][1].view(torch.int32))
            print(json.dumps({"measure": "topk_routes", "Q": Q, "N": N, "E": E, "k": k, "few_query": _stats(ms[2], N * E * 4),
                              "wide": _stats(ms[1], N * E * 4),
                              "few_query_over_wide": round(float(np.median(ms[2]) / np.median(ms[1])), 3)}), flush=True)
    finally:
        _lib.check(L.clipgpu_test_topk_route(0))
        ix.close()


def topk_filter_leg(N=1 << 20, E=512, k=10, runs=7, warmup=2, Qs=(1, 16, 256)):
    """What an allow bitmap costs and saves (clipgpu_index_search_filtered_device, f32 gallery): six legs
    alternate in one process, their order rotating from round to round -- the unfiltered search, and the
    filtered search under a bitmap of all ones (the overhead of the mask), a random 50 % and a random 1 %
    of the rows (no 64-column tile is empty: nothing to skip), and one contiguous range of 10 % of the rows
    (whole spans are empty), and the same result by the full-matrix path (clipgpu_similarity_device logits,
    masked_fill(-inf), torch.topk; timed under the 50 % bitmap).  Per leg the median and the spread of
    `runs` device-event timings after `warmup` rounds.  Every fused leg returns the indices and the
    bit-equal scores of the full-matrix path under its bitmap (computed once more, untimed, per bitmap)."""
    import ctypes
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.index import pack_allow
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.nn.functional.normalize(torch.randn(N, E, device="cuda"), dim=1)
    allows = {"all_ones": np.ones(N, bool), "random_50pct": rng.random(N) < 0.5, "random_1pct": rng.random(N) < 0.01,
              "range_10pct": (np.arange(N) >= N // 3) & (np.arange(N) < N // 3 + N // 10)}
    d_bool = {name: torch.from_numpy(a).cuda() for name, a in allows.items()}
    d_words = {name: torch.from_numpy(pack_allow(a).view(np.int32)).cuda() for name, a in allows.items()}
    ix = EmbeddingIndex(E, N)
    ix.add_device(g.data_ptr(), N, s)
    try:
        for Q in Qs:
            q = torch.nn.functional.normalize(torch.randn(Q, E, device="cuda"), dim=1)
            mat = torch.empty(Q, N, device="cuda")
            names = ["unfiltered"] + list(allows)
            res = {name: (torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((Q, k), device="cuda"))
                   for name in names}

            def fused(name):
                ix.search_device(q.data_ptr(), Q, k, res[name][0].data_ptr(), res[name][1].data_ptr(), 100.0, 0.0, s,
                                 d_allow=0 if name == "unfiltered" else d_words[name].data_ptr())

            def baseline(name="random_50pct"):
                _lib.check(L.clipgpu_similarity_device(ctypes.c_void_p(q.data_ptr()), Q, ctypes.c_void_p(g.data_ptr()),
                                                       N, E, 100.0, 0.0, 2, 1, ctypes.c_void_p(mat.data_ptr()),
                                                       ctypes.c_void_p(s)))
                if name != "unfiltered":
                    mat.masked_fill_(~d_bool[name][None, :], float("-inf"))
                return torch.topk(mat, k, dim=1)

            legs = tuple((name, (lambda n=name: fused(n))) for name in names) + (("baseline", baseline),)
            ms = {name: [] for name, _ in legs}
            for rnd in range(warmup + runs):
                r = rnd % len(legs)
                for name, fn in legs[r:] + legs[:r]:  # every leg follows every other equally often
                    t = _event_ms(fn)
                    if rnd >= warmup:
                        ms[name].append(t)
            for name in names:  # the same result: scores bit for bit; indices once the baseline's ties are in index order
                b_score, b_idx = (x.cpu().numpy() for x in baseline(name))
                order = np.lexsort((b_idx, -b_score.astype(np.float64)), axis=1)
                b_idx, b_score = np.take_along_axis(b_idx, order, 1), np.take_along_axis(b_score, order, 1)
                assert np.array_equal(res[name][1].cpu().numpy().view(np.uint32), b_score.view(np.uint32)), name
                assert np.array_equal(res[name][0].cpu().numpy(), b_idx), name
            nbytes = N * E * 4
            out = {"measure": "topk_filter", "Q": Q, "N": N, "E": E, "k": k, "runs": runs, "same_as_baseline": True,
                   "allowed_rows": {name: int(a.sum()) for name, a in allows.items()}}
            for name, v in ms.items():
                out[name] = _stats(v, nbytes)
            for name in allows:
                out[name + "_over_unfiltered"] = round(out[name]["ms_median"] / out["unfiltered"]["ms_median"], 3)
            print(json.dumps(out), flush=True)
    finally:
        ix.close()


def topk_probs_leg(N=1 << 20, E=512, k=10, runs=7, warmup=2, Qs=(1, 16, 256), dtypes=("f32", "f16")):
    """What the probabilities cost (clipgpu_index_search_probs_device, softmax, scale 100): three legs
    alternate in one process, their order rotating from round to round -- the probability search, the plain
    search, and the same result by the full-matrix path (clipgpu_similarity_device softmax over the gallery
    of each query into a [Q][N] tensor, then torch.topk of the probabilities: the softmax is monotone, so
    no gather by the logits' order is needed), which for a 16-bit index runs on the widened rounded gallery.  Per leg the median and the spread of `runs` device-event timings after `warmup`
    rounds.  The probability search returns the plain search's indices and bit-equal logits; its
    probabilities are compared with the matrix path's at the same indices (largest relative difference in
    the line; tests/test_gpu_index_probs.py holds them to the derived bound at small shapes)."""
    import ctypes
    from open_clip_inference import EmbeddingIndex
    torch.manual_seed(0)
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.nn.functional.normalize(torch.randn(N, E, device="cuda"), dim=1)
    qs = {Q: torch.nn.functional.normalize(torch.randn(Q, E, device="cuda"), dim=1) for Q in Qs}
    for dt in dtypes:
        esz, tdt = INDEX_DTYPES[dt]
        gw = g if tdt is None else g.to(tdt).float()  # what the index holds, widened
        ix = EmbeddingIndex(E, N, dtype=dt)
        ix.add_device(g.data_ptr(), N, s)
        try:
            for Q in Qs:
                q = qs[Q]
                mat = torch.empty(Q, N, device="cuda")
                idx = {n: torch.empty((Q, k), dtype=torch.int64, device="cuda") for n in ("probs", "plain")}
                score = {n: torch.empty((Q, k), device="cuda") for n in ("probs", "plain")}
                prob, norm = torch.empty((Q, k), device="cuda"), torch.empty((Q, 2), device="cuda")
                base = {}

                def probs():
                    ix.search_probs_device(q.data_ptr(), Q, k, idx["probs"].data_ptr(), score["probs"].data_ptr(),
                                           prob.data_ptr(), 100.0, 0.0, "softmax", s, d_norm=norm.data_ptr())

                def plain():
                    ix.search_device(q.data_ptr(), Q, k, idx["plain"].data_ptr(), score["plain"].data_ptr(), 100.0, 0.0, s)

                def baseline():
                    _lib.check(L.clipgpu_similarity_device(ctypes.c_void_p(q.data_ptr()), Q, ctypes.c_void_p(gw.data_ptr()),
                                                           N, E, 100.0, 0.0, 0, 1, ctypes.c_void_p(mat.data_ptr()),
                                                           ctypes.c_void_p(s)))
                    base["prob"], base["idx"] = torch.topk(mat, k, dim=1)

                legs = (("probs", probs), ("plain", plain), ("baseline", baseline))
                ms = {name: [] for name, _ in legs}
                for rnd in range(warmup + runs):
                    for name, fn in legs[rnd % 3:] + legs[:rnd % 3]:  # every leg follows every other equally often
                        t = _event_ms(fn)
                        if rnd >= warmup:
                            ms[name].append(t)
                assert torch.equal(idx["probs"], idx["plain"])
                assert torch.equal(score["probs"].view(torch.int32), score["plain"].view(torch.int32))
                want = torch.gather(mat, 1, idx["probs"])  # the matrix path's probabilities of the same rows
                rel = float(((prob - want).abs() / want.clamp_min(1e-30)).max())
                nbytes = N * E * esz
                out = {"measure": "topk_probs", "Q": Q, "dtype": dt, "N": N, "E": E, "k": k, "runs": runs,
                       "same_indices_and_logits_as_plain": True, "max_rel_diff_vs_matrix_softmax": float(f"{rel:.3g}"),
                       "same_top1_as_matrix": bool(torch.equal(base["idx"][:, 0], idx["probs"][:, 0]))}
                for name, v in ms.items():
                    out[name] = _stats(v, nbytes)
                out["probs_over_plain"] = round(out["probs"]["ms_median"] / out["plain"]["ms_median"], 3)
                out["probs_over_baseline"] = round(out["probs"]["ms_median"] / out["baseline"]["ms_median"], 3)
                print(json.dumps(out), flush=True)
        finally:
            ix.close()


def latency_leg(steps=50, warmup=10):
    """Single-item latency (the reference's embed_image / embed_text calls, B = 1) through the
    host entry points: pinned staging + H2D + forward + D2H + synchronise, ViT-B/32."""
    d = model_dir(VIT_B_32_CFG)
    mean, std = VIT_B_32_CFG["preprocess_cfg"]["mean"], VIT_B_32_CFG["preprocess_cfg"]["std"]
    ve = Engine(d, 0, [0], "bf16", 8)
    te = Engine(d, 1, [0], "bf16", 8)
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (1, 224, 224, 3), dtype=np.uint8)
    px = np.ascontiguousarray(((u8.astype(np.float32) / 255 - np.asarray(mean, np.float32)) /
                               np.asarray(std, np.float32)).transpose(0, 3, 1, 2))
    ids = np.zeros((1, 77), np.int64)
    ids[0, :5] = [49406, 320, 1125, 539, 49407]
    photo = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)]
    for name, fn in (("b32_embed_image_f32", lambda: ve.embed_pixels(px)),
                     ("b32_embed_image_photo_gpu_resize", lambda: ve.embed_images_rgb8(photo)),
                     ("b32_embed_text", lambda: te.embed_tokens(ids))):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        print(json.dumps({"measure": "latency_" + name, "batch": 1, "p50_ms": round(ts[len(ts) // 2] * 1e3, 3),
                          "p90_ms": round(ts[int(len(ts) * 0.9)] * 1e3, 3)}), flush=True)
    ve.close()
    te.close()


if __name__ == "__main__":
    which = sys.argv[1:] or ["host", "photos", "similarity", "latency", "so400m", "h14"]
    if "host" in which:
        host_leg()
    if "captions" in which:
        captions_leg()
    if "photos" in which:
        photos_leg()
    if "similarity" in which:
        similarity_leg()
    if "latency" in which:
        latency_leg()
    if "topk" in which:  # the embedding index's fused search vs similarity + torch.topk
        topk_leg()
    if "topkroutes" in which:  # the few-query kernel vs the wide one per query count: sets kNarrowRows
        topk_routes_leg()
    if "topkfilter" in which:  # the filtered search: the cost of the mask and the gain from the skips
        topk_filter_leg()
    if "topkprobs" in which:  # the probability search against the plain search and the matrix softmax + topk
        topk_probs_leg()
    if "topkrange" in which:  # the range search against search k = 10, dense emission, and the self-join
        topk_range_leg()
    if "kmeans" in which:  # one k-means iteration: assign against the range search, the integer-sum update
        kmeans_leg()
    if "ivf" in which:  # the probed search against the plain search on a clustered gallery
        ivf_leg()
    if "codes" in which:  # the coded search (int8 scan + exact re-rank) against the plain search
        codes_leg()
    if "so400m" in which:
        device_leg("so400m_vision", SO400M_16_SIGLIP2_384_CFG, 0, 128)
    if "h14" in which:
        device_leg("h14_vision", VIT_H_14_378_CFG, 0, 64)
        device_leg("h14_text", VIT_H_14_378_CFG, 1, 64)
    if "h14fp8" in which:
        # configs[4]'s fp8 MFMA weight path at the north-star tolerance: vision with
        # QKV in MX-fp8 (cos >= 0.9999), text in bf16 -- no MX text split meets the bar at any
        # speed gain (per-site and per-layer sweeps, profiles/r04_mx_layer_*.jsonl)
        device_leg("h14_vision_fp8", VIT_H_14_378_CFG, 0, 64, dtype="fp8", mx_sites="qkv")
        device_leg("h14_text", VIT_H_14_378_CFG, 1, 64)
    if "h14fp8full" in which:  # the full MX split (QKV, c_fc, c_proj): throughput mode, below the bar
        device_leg("h14_vision_fp8_full", VIT_H_14_378_CFG, 0, 64, dtype="fp8")
        device_leg("h14_text_fp8_full", VIT_H_14_378_CFG, 1, 64, dtype="fp8")
    if "lanesab" in which:  # one vs two device lanes at the large-model shards (table tiles), interleaved
        for rnd in range(2):
            for lanes in (1, 2):
                device_leg("so400m_vision", SO400M_16_SIGLIP2_384_CFG, 0, 128, lanes=lanes)
                device_leg("h14_vision", VIT_H_14_378_CFG, 0, 64, lanes=lanes)
                device_leg("h14_text", VIT_H_14_378_CFG, 1, 64, lanes=lanes)
    if "so400mtext" in which:  # the SigLIP2 text tower of the configs[3] model folder
        device_leg("so400m_text", SO400M_16_SIGLIP2_384_CFG, 1, 128)
    if "so400mfp8" in which:
        device_leg("so400m_vision_fp8", SO400M_16_SIGLIP2_384_CFG, 0, 128, dtype="fp8")
    if "b32fp8" in which:
        device_leg("b32_vision_fp8", VIT_B_32_CFG, 0, 256, dtype="fp8")
