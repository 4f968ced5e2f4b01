// What a replica holds on its device: the weight upload (with the LayerNorm fold), the workspace
// layout, and the teardown of both.
#include "engine.hpp"

namespace clipgpu {

namespace {

const HostTensor& need(const TensorMap& m, const std::string& k) {
  auto it = m.find(k);
  if (it == m.end()) throw ClipErr(CLIPGPU_ERR_CONFIG, "Configuration error: missing tensor " + k);
  return it->second;
}

// Bump allocator over a device arena.
struct Bump {
  char* base;
  size_t off = 0;
  size_t cap;
  void* take(size_t n) {
    void* p = base + off;
    off += align256(n);
    if (off > cap) throw ClipErr(CLIPGPU_ERR_DEVICE, "internal: arena overflow");
    return p;
  }
};

size_t weight_bytes(const TowerSpec& s, const TensorMap& m) {
  size_t total = 0;
  for (const ParamDesc& p : tower_params(s)) total += align256((size_t)need(m, p.name).numel() * 4);
  // zero padding of the MLP hidden width and of the patch K (16-bit matrices + f32 bias)
  const size_t mpad = (size_t)(mlp_pad(s) - s.mlp_width);
  total += (size_t)s.layers * (mpad * s.width * 4 + mpad * 4 + 1024);
  if (s.tower == TOWER_VISION) total += (size_t)(kpatch_pad(s) - kpatch(s)) * s.width * 2 + 256;
  if (s.family == FAMILY_SIGLIP) total += (mpad * s.width * 4 + mpad * 4) + (size_t)s.width * 4 + 4096;
  return total + 4096;
}

void upload_f32(const HostTensor& t, float* dst) {
  HIP_CHECK(copy_h2d(dst, t.data.data(), t.data.size() * 4));
}

void upload_16(DType dt, const float* src, size_t n, void* dst, float* staging, hipStream_t s) {
  HIP_CHECK(copy_h2d(staging, src, n * 4));
  HIP_CHECK(launch_cast_f32(dt, staging, dst, (long)n, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// The upload's f32 device staging buffers: freed on every exit of upload_weights, a throw included.
struct Staging {
  std::vector<float*> bufs;
  float* take(size_t n) {
    float* p = nullptr;
    HIP_CHECK(hipMalloc(&p, n * 4));
    bufs.push_back(p);
    return p;
  }
  ~Staging() {
    for (float* p : bufs) (void)hipFree(p);
  }
};

}  // namespace

void upload_weights(clipgpu_engine& e, Replica& r, const TensorMap& m) {
  const TowerSpec& s = e.spec;
  const size_t bytes = weight_bytes(s, m);
  HIP_CHECK(hipMalloc(&r.arena, bytes));
  Bump a{r.arena, 0, bytes};
  const int D = s.width;
  size_t max16 = 0;
  for (const ParamDesc& p : tower_params(s)) max16 = std::max(max16, (size_t)need(m, p.name).numel());
  Staging stg;
  float* const staging = stg.take(max16);
  auto staging_pad = [&](size_t n) {  // a padded matrix may exceed max16
    return n <= max16 ? staging : stg.take(n);
  };
  auto f32 = [&](const std::string& k) {
    const HostTensor& t = need(m, k);
    float* p = (float*)a.take(t.data.size() * 4);
    upload_f32(t, p);
    return p;
  };
  auto w16 = [&](const std::string& k) {
    const HostTensor& t = need(m, k);
    void* p = a.take(t.data.size() * 2);
    upload_16(e.dt, t.data.data(), t.data.size(), p, staging, r.stream);
    return p;
  };
  // [R][C] -> zero-padded [Rp][Cp] on the host (empty: the tensor has that shape already)
  auto padded = [&](const HostTensor& t, int64_t Rp, int64_t Cp) {
    const int64_t R = t.shape[0], C = t.numel() / t.shape[0];
    std::vector<float> pad;
    if (Rp == R && Cp == C) return pad;
    pad.assign((size_t)(Rp * Cp), 0.f);
    for (int64_t i = 0; i < R; ++i) std::memcpy(&pad[(size_t)(i * Cp)], &t.data[(size_t)(i * C)], (size_t)C * 4);
    return pad;
  };
  // [R][C] -> zero-padded [Rp][Cp] (16-bit)
  auto w16_pad = [&](const std::string& k, int64_t Rp, int64_t Cp) {
    const std::vector<float> pad = padded(need(m, k), Rp, Cp);
    if (pad.empty()) return w16(k);
    void* p = a.take(pad.size() * 2);
    upload_16(e.dt, pad.data(), pad.size(), p, staging_pad(pad.size()), r.stream);
    return p;
  };
  // [R][C] f32 -> zero-padded [Rp][Cp] MX-fp8 (quantized on the device)
  auto wmx_pad = [&](const std::string& k, int64_t Rp, int64_t Cp) {
    const HostTensor& t = need(m, k);
    const std::vector<float> pad = padded(t, Rp, Cp);
    const float* src = pad.empty() ? t.data.data() : pad.data();
    float* stg = staging_pad((size_t)(Rp * Cp));
    HIP_CHECK(copy_h2d(stg, src, (size_t)(Rp * Cp) * 4));
    MxW w;
    w.q = (uint8_t*)a.take((size_t)(Rp * Cp));
    w.s = (uint8_t*)a.take((size_t)(Rp * Cp / 32));
    HIP_CHECK(launch_quant_rows(-1, stg, Cp, w.q, Cp, w.s, Cp / 32, (int)Rp, (int)Cp, r.stream));
    HIP_CHECK(hipStreamSynchronize(r.stream));
    return w;
  };
  auto f32_pad = [&](const std::string& k, int64_t n) {
    const HostTensor& t = need(m, k);
    std::vector<float> pad((size_t)n, 0.f);
    std::memcpy(pad.data(), t.data.data(), t.data.size() * 4);
    float* p = (float*)a.take(pad.size() * 4);
    HIP_CHECK(copy_h2d(p, pad.data(), pad.size() * 4));
    return p;
  };
  auto a_take_f32 = [&](const std::vector<float>& v) {
    float* p = (float*)a.take(v.size() * 4);
    HIP_CHECK(copy_h2d(p, v.data(), v.size() * 4));
    return p;
  };
  auto w16_transposed = [&](const std::string& k) {  // [D][E] -> [E][D]
    const HostTensor& t = need(m, k);
    const int64_t R = t.shape[0], C = t.shape[1];
    std::vector<float> tr((size_t)(R * C));
    for (int64_t i = 0; i < R; ++i)
      for (int64_t j = 0; j < C; ++j) tr[(size_t)(j * R + i)] = t.data[(size_t)(i * C + j)];
    void* p = a.take(tr.size() * 2);
    upload_16(e.dt, tr.data(), tr.size(), p, staging, r.stream);
    return p;
  };
  DevWeights& w = r.w;
  std::string pre;
  const bool siglip = s.tower == TOWER_VISION && s.family == FAMILY_SIGLIP;
  // parameter names of the two families (open_clip CLIP / timm ViT trunk)
  const char* n_ln1w = siglip ? "norm1.weight" : "ln_1.weight";
  const char* n_ln1b = siglip ? "norm1.bias" : "ln_1.bias";
  const char* n_qkvw = siglip ? "attn.qkv.weight" : "attn.in_proj_weight";
  const char* n_qkvb = siglip ? "attn.qkv.bias" : "attn.in_proj_bias";
  const char* n_ow = siglip ? "attn.proj.weight" : "attn.out_proj.weight";
  const char* n_ob = siglip ? "attn.proj.bias" : "attn.out_proj.bias";
  const char* n_ln2w = siglip ? "norm2.weight" : "ln_2.weight";
  const char* n_ln2b = siglip ? "norm2.bias" : "ln_2.bias";
  const char* n_fc1w = siglip ? "mlp.fc1.weight" : "mlp.c_fc.weight";
  const char* n_fc1b = siglip ? "mlp.fc1.bias" : "mlp.c_fc.bias";
  const char* n_fc2w = siglip ? "mlp.fc2.weight" : "mlp.c_proj.weight";
  const char* n_fc2b = siglip ? "mlp.fc2.bias" : "mlp.c_proj.bias";
  if (siglip) {
    const std::string t = "visual.trunk.";
    w.conv_w = w16_pad(t + "patch_embed.proj.weight", D, kpatch_pad(s));
    w.conv_b = f32(t + "patch_embed.proj.bias");
    w.pos = f32(t + "pos_embed");
    pre = t + "blocks.";
  } else if (s.tower == TOWER_VISION) {
    w.conv_w = w16_pad("visual.conv1.weight", D, kpatch_pad(s));
    w.cls = f32("visual.class_embedding");
    w.pos = f32("visual.positional_embedding");
    w.lnpre_w = f32("visual.ln_pre.weight");
    w.lnpre_b = f32("visual.ln_pre.bias");
    pre = "visual.transformer.resblocks.";
  } else {
    w.tok = f32("token_embedding.weight");
    w.pos = f32("positional_embedding");
    pre = "transformer.resblocks.";
  }
  // LayerNorm fold (clipgpu_engine::lnf) of the GEMM W [R][D] + b behind LayerNorm (gamma, beta):
  // W' = f16(W diag(gamma)) zero-padded to Rp rows, bias b + W beta (f64 sums, the f32 W), and the
  // column sums of W' as the kernel sees it (f16-rounded; f64 sums): LN(x) W^T + b =
  // rstd (x W'^T - mean cs) + b + W beta.
  auto fold_w = [&](const std::string& wk, const std::string& bk, const std::string& gk, const std::string& bek,
                    int64_t Rp, void*& wout, float*& bout, float*& csout) {
    const HostTensor& W = need(m, wk);
    const HostTensor& b = need(m, bk);
    const HostTensor& g = need(m, gk);
    const HostTensor& be = need(m, bek);
    const int64_t R = W.shape[0], C = W.numel() / W.shape[0];
    std::vector<float> wf((size_t)(Rp * C), 0.f), cs((size_t)Rp, 0.f), bp((size_t)Rp, 0.f);
    for (int64_t i = 0; i < R; ++i) {
      double sb = b.data[(size_t)i], sc = 0.0;
      for (int64_t k = 0; k < C; ++k) {
        const float wv = W.data[(size_t)(i * C + k)];
        const float wg = wv * g.data[(size_t)k];
        wf[(size_t)(i * C + k)] = wg;
        sc += (double)(float)(_Float16)wg;  // the device cast's rounding (to nearest even)
        sb += (double)wv * (double)be.data[(size_t)k];
      }
      cs[(size_t)i] = (float)sc;
      bp[(size_t)i] = (float)sb;
    }
    wout = a.take(wf.size() * 2);
    upload_16(DT_F16, wf.data(), wf.size(), wout, staging_pad(wf.size()), r.stream);
    bout = a_take_f32(bp);
    csout = a_take_f32(cs);
  };
  for (int l = 0; l < s.layers; ++l) {
    const std::string p = pre + std::to_string(l) + ".";
    LayerW L;
    L.ln1_w = f32(p + n_ln1w);
    L.ln1_b = f32(p + n_ln1b);
    L.wqkv = L.w1 = L.w2 = nullptr;
    if (e.lnf) fold_w(p + n_qkvw, p + n_qkvb, p + n_ln1w, p + n_ln1b, 3 * D, L.wqkv, L.bqkv, L.cs_qkv);
    else if (mx_at(e, l, GS_QKV)) L.mqkv = wmx_pad(p + n_qkvw, 3 * D, D);
    else L.wqkv = w16(p + n_qkvw);
    if (e.lnf) fold_w(p + n_fc1w, p + n_fc1b, p + n_ln2w, p + n_ln2b, mlp_pad(s), L.w1, L.b1, L.cs_1);
    else if (mx_at(e, l, GS_FC)) L.m1 = wmx_pad(p + n_fc1w, mlp_pad(s), D);
    else L.w1 = w16_pad(p + n_fc1w, mlp_pad(s), D);
    if (mx_at(e, l, GS_PROJ)) L.m2 = wmx_pad(p + n_fc2w, D, mlp_pad(s));
    else L.w2 = w16_pad(p + n_fc2w, D, mlp_pad(s));
    if (!e.lnf) L.bqkv = f32(p + n_qkvb);
    L.wo = w16(p + n_ow);
    L.bo = f32(p + n_ob);
    L.ln2_w = f32(p + n_ln2w);
    L.ln2_b = f32(p + n_ln2b);
    if (!e.lnf) L.b1 = f32_pad(p + n_fc1b, mlp_pad(s));
    L.b2 = f32(p + n_fc2b);
    w.layers.push_back(L);
  }
  if (siglip) {
    const std::string t = "visual.trunk.", a = "visual.trunk.attn_pool.";
    w.lnpost_w = f32(t + "norm.weight");  // final norm, before the attention pool
    w.lnpost_b = f32(t + "norm.bias");
    {  // q = latent . Wq^T + bq, shared by every image (f64 accumulation)
      const HostTensor& lat = need(m, a + "latent");
      const HostTensor& wq = need(m, a + "q.weight");
      const HostTensor& bq = need(m, a + "q.bias");
      std::vector<float> q((size_t)D);
      for (int j = 0; j < D; ++j) {
        double acc = bq.data[(size_t)j];
        for (int i = 0; i < D; ++i) acc += (double)lat.data[(size_t)i] * wq.data[(size_t)j * D + i];
        q[(size_t)j] = (float)acc;
      }
      w.map.q = (float*)a_take_f32(q);
    }
    w.map.wkv = w16(a + "kv.weight");
    w.map.bkv = f32(a + "kv.bias");
    w.map.wproj = w16(a + "proj.weight");
    w.map.bproj = f32(a + "proj.bias");
    w.map.norm_w = f32(a + "norm.weight");
    w.map.norm_b = f32(a + "norm.bias");
    w.map.w1 = w16_pad(a + "mlp.fc1.weight", mlp_pad(s), D);
    w.map.b1 = f32_pad(a + "mlp.fc1.bias", mlp_pad(s));
    w.map.w2 = w16_pad(a + "mlp.fc2.weight", D, mlp_pad(s));
    w.map.b2 = f32(a + "mlp.fc2.bias");
  } else if (s.tower == TOWER_VISION) {
    w.lnpost_w = f32("visual.ln_post.weight");
    w.lnpost_b = f32("visual.ln_post.bias");
    w.proj_t = w16_transposed("visual.proj");
  } else {
    w.lnpost_w = f32("ln_final.weight");
    w.lnpost_b = f32("ln_final.bias");
    if (s.proj_bias) {  // nn.Linear: weight already [E][D]
      w.proj_t = w16("text_projection.weight");
      w.proj_b = f32("text_projection.bias");
    } else {
      w.proj_t = w16_transposed("text_projection");
    }
  }
}

void alloc_workspace(clipgpu_engine& e, Replica& r) {
  const TowerSpec& s = e.spec;
  // lanes x ceil(max_batch / lanes) rows: every host-path slot (run_host_shard) is whole
  const size_t B = (size_t)((e.max_batch + e.lanes - 1) / e.lanes * e.lanes);
  const size_t rows = B * (size_t)s.tokens(), D = s.width;
  const size_t wide = big_wide(s);
  const size_t E = s.embed_dim;
  const size_t MLP = (size_t)mlp_pad(s);
  const size_t sizes[] = {rows * D * 4, rows * D * 2, rows * wide * 2, B * D * 2, B * E * 4, B * E * 4,
                          B * e.in_bytes_per_row, e.mx ? rows * D / 32 : 0, e.mx ? rows * MLP / 32 : 0,
                          (rows + 256) * 8};
  size_t total = 0;
  for (size_t z : sizes) total += align256(z);
  HIP_CHECK(hipMalloc(&r.work, total));
  HIP_CHECK(hipMemset(r.work, 0, total));
  Bump a{r.work, 0, total};
  r.x = a.take(sizes[0]);  // f32 capacity (an f16 stream uses the first half)
  r.h = a.take(sizes[1]);
  r.big = a.take(sizes[2]);
  r.pooled = a.take(sizes[3]);
  r.emb = (float*)a.take(sizes[4]);
  HostSet& hs = r.hset[0];
  hs.out = (float*)a.take(sizes[5]);
  hs.in = a.take(sizes[6]);
  r.hs = e.mx ? (uint8_t*)a.take(sizes[7]) : nullptr;
  r.bigs = e.mx ? (uint8_t*)a.take(sizes[8]) : nullptr;
  r.xs = (float*)a.take(sizes[9]);
  for (int i = 0; i < e.lanes; ++i) {
    HIP_CHECK(hipStreamCreateWithFlags(&r.lane[i], hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&r.join[i], hipEventDisableTiming));
  }
  for (int i = 0; i < 4; ++i) {  // host-path chunks: up to 4 (host_chunks), independent of the lanes
    HIP_CHECK(hipEventCreateWithFlags(&hs.done[i], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&hs.copied[i], hipEventDisableTiming));
  }
  HIP_CHECK(hipStreamCreateWithFlags(&r.copy, hipStreamNonBlocking));
  HIP_CHECK(hipStreamCreateWithFlags(&r.copy2, hipStreamNonBlocking));
  HIP_CHECK(hipEventCreateWithFlags(&r.fork, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&r.gin, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&r.gout, hipEventDisableTiming));
  r.graphs = new GraphCache();
  HIP_CHECK(hipHostMalloc(&hs.pin_in, B * e.in_bytes_per_row, hipHostMallocDefault));
  HIP_CHECK(hipHostMalloc((void**)&hs.pin_out, B * E * 4, hipHostMallocDefault));
}

// Releases whatever the replica holds, a partly built one (a failed clipgpu_create_ex) included.
void destroy_replica(Replica& r) {
  if (!r.stream) return;  // never built: the stream is a replica's first resource
  (void)hipSetDevice(r.device);
  // every stream of the replica (lanes, copy streams: a device-path call's forks may still run) is idle
  // before its memory goes
  (void)hipDeviceSynchronize();
  if (r.arena) (void)hipFree(r.arena);
  if (r.work) (void)hipFree(r.work);
  for (HostSet& hs : r.hset) {
    if (hs.pin_in) (void)hipHostFree(hs.pin_in);
    if (hs.pin_out) (void)hipHostFree(hs.pin_out);
    if (hs.owns_device && hs.in) (void)hipFree(hs.in);
    if (hs.owns_device && hs.out) (void)hipFree(hs.out);
  }
  if (r.stream) (void)hipStreamDestroy(r.stream);
  if (r.copy) (void)hipStreamDestroy(r.copy);
  if (r.copy2) (void)hipStreamDestroy(r.copy2);
  for (int i = 0; i < 4; ++i) {
    if (r.lane[i]) (void)hipStreamDestroy(r.lane[i]);
    if (r.join[i]) (void)hipEventDestroy(r.join[i]);
    for (HostSet& hs : r.hset) {
      if (hs.done[i]) (void)hipEventDestroy(hs.done[i]);
      if (hs.copied[i]) (void)hipEventDestroy(hs.copied[i]);
    }
  }
  if (r.fork) (void)hipEventDestroy(r.fork);
  if (r.gin) (void)hipEventDestroy(r.gin);
  if (r.gout) (void)hipEventDestroy(r.gout);
  if (r.coll) (void)hipEventDestroy(r.coll);
  if (r.graphs) {
    r.graphs->clear();
    delete r.graphs;
  }
  for (auto& sl : r.islot) {
    if (sl.pin) (void)hipHostFree(sl.pin);
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.tmp) (void)hipFree(sl.tmp);
  }
  r = Replica();
}

}  // namespace clipgpu
