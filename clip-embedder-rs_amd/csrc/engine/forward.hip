// The forward of one tower on one replica: the trunk's GEMM sites, the trunk, the heads, the two
// towers' stems, and the concurrent lanes.
#include "engine.hpp"

namespace clipgpu {

namespace {

// Times the launches of one scope when its category is enabled.  gemm = true (a single
// launch_gemm inside): the events are handed to the GEMM launcher, which stamps the kernel's
// own start and end (hipExtLaunchKernelGGL); otherwise [start, stop] are recorded around the
// scope's launches on the stream (which also counts their dispatch gaps).
struct ProfScope {
  Profiler* p;
  int cat;
  hipStream_t st;
  bool gemm;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(const clipgpu_engine& e, int c, hipStream_t s, bool gemm_scope = false)
      : p(const_cast<Profiler*>(&e.prof)), cat(c), st(s), gemm(gemm_scope) {
    if (p->mask & (1u << cat)) {
      a = p->get();
      b = a ? p->get() : nullptr;
      if (!b) {
        a = nullptr;
      } else if (gemm) {
        g_gemm_events.start = a;
        g_gemm_events.stop = b;
      } else {
        (void)hipEventRecord(a, st);
      }
    }
  }
  ~ProfScope() {
    if (!a) return;
    if (gemm) g_gemm_events = GemmLaunchEvents();  // consumed by the launch (or disarm on error)
    else (void)hipEventRecord(b, st);
    p->pending.push_back({cat, a, b, st});
  }
};

GemmParams rows_gemm(const void* A, long lda, const void* W, const float* bias, void* out, long ldo, int M, int N,
                     int K) {
  GemmParams g{};
  g.A = A;
  g.lda = lda;
  g.W = W;
  g.ldw = K;
  g.bias = bias;
  g.out = out;
  g.ldo = ldo;
  g.M = M;
  g.N = N;
  g.K = K;
  return g;
}

}  // namespace

SiteShape site_shape(const clipgpu_engine& e, int site) {
  const int D = e.spec.width, MLP = mlp_pad(e.spec);
  switch (site) {
    case GS_QKV: return {3 * D, D};
    case GS_OUT: return {D, D};
    case GS_FC: return {MLP, D};
    default: return {D, MLP};
  }
}

int site_epi(const clipgpu_engine& e, int site) {
  if (site == GS_OUT || site == GS_PROJ) return EPI_RESID;
  return e.lnf ? EPI_LNF : EPI_STORE16;  // QKV / c_fc behind the folded LayerNorm
}

// Tile order per trunk site (GemmParams.group: row panels per group, 0 = the kernels' 8).  qkv and
// c_proj walk N first (group 1): their W (3 D x D, D x MLP) is small beside A, so each XCD reads an A
// row panel once and all of W, instead of every panel from two XCDs: c_proj's fetched bytes at the
// ViT-B/32 lane shape drop from 1.96x to ~1.4x its compulsory bytes.  Speed
// only: the order never changes a tile's sums.  (CLIPGPU_SITE_GROUPS=0 builds the uniform order for
// A/B runs.)
#ifndef CLIPGPU_SITE_GROUPS
#define CLIPGPU_SITE_GROUPS 1
#endif
constexpr int kSiteGroup[4] = {CLIPGPU_SITE_GROUPS ? 1 : 0, 0, 0, CLIPGPU_SITE_GROUPS ? 1 : 0};

GemmParams site_gemm(const clipgpu_engine& e, const Replica& r, const LayerW& L, int site, int rows) {
  const int D = e.spec.width, MLP = mlp_pad(e.spec);
  GemmParams g;
  // (LayerNorm-folded engines: QKV and c_fc read the residual stream x itself, EPI_LNF)
  const void* ln_in = e.lnf ? r.x : r.h;
  switch (site) {
    case GS_QKV: g = rows_gemm(ln_in, D, L.wqkv, L.bqkv, r.big, 3 * D, rows, 3 * D, D); break;
    case GS_OUT: g = rows_gemm(r.h, D, L.wo, L.bo, r.x, D, rows, D, D); break;
    case GS_FC: g = rows_gemm(ln_in, D, L.w1, L.b1, r.big, MLP, rows, MLP, D); break;
    default: g = rows_gemm(r.big, MLP, L.w2, L.b2, r.x, D, rows, D, MLP); break;
  }
  if (e.lnf && (site == GS_QKV || site == GS_FC)) {
    g.cs = site == GS_QKV ? L.cs_qkv : L.cs_1;
    g.rowstats = r.xs;
  }
  g.group = kSiteGroup[site];
  g.x16 = e.x16 ? 1 : 0;
  // the younger half of 8-wave blocks at priority 1: vision +0.75 %, text -0.5 % (gemm.hip)
  g.prio = e.spec.tower == TOWER_VISION ? 1 : 0;
  return g;
}

// fp8 engines: the MX-fp8 GEMM of a trunk site (QKV: LN e4m3 -> 16-bit qkv; c_fc: LN e4m3 ->
// act -> e4m3 hidden in `big` + scales; c_proj: e4m3 hidden -> residual stream).
// c_fc quantizes its output (EPI_STOREQ) only when the layer's c_proj consumes MX; else it stores 16-bit.
int site_epi_mx(const clipgpu_engine& e, int l, int site) {
  return site == GS_PROJ ? EPI_RESID : (site == GS_FC && mx_at(e, l, GS_PROJ) ? EPI_STOREQ : EPI_STORE16);
}
// LN output feeding an MX GEMM (layer l's consumer site) is written as MX-fp8 (scales in hs), else 16-bit.
static inline uint8_t* ln_q(const clipgpu_engine& e, int l, int consumer_site, uint8_t* hs) {
  return mx_at(e, l, consumer_site) ? hs : nullptr;
}

MxGemmParams site_gemm_mx(const clipgpu_engine& e, const Replica& r, const LayerW& L, int site, int rows) {
  const int D = e.spec.width, MLP = mlp_pad(e.spec);
  MxGemmParams g{};
  g.M = rows;
  if (site == GS_PROJ) {
    g.A = (const uint8_t*)r.big; g.lda = MLP; g.As = r.bigs; g.ldas = MLP / 32;
    g.W = L.m2.q; g.ldw = MLP; g.Ws = L.m2.s; g.ldws = MLP / 32;
    g.bias = L.b2; g.out = r.x; g.ldo = D; g.N = D; g.K = MLP;
    g.x16 = e.x16 ? 1 : 0;
    return g;
  }
  g.A = (const uint8_t*)r.h; g.lda = D; g.As = r.hs; g.ldas = D / 32;
  g.K = D;
  if (site == GS_QKV) {
    g.W = L.mqkv.q; g.ldw = D; g.Ws = L.mqkv.s; g.ldws = D / 32;
    g.bias = L.bqkv; g.out = r.big; g.ldo = 3 * D; g.N = 3 * D;
  } else {  // GS_FC
    g.W = L.m1.q; g.ldw = D; g.Ws = L.m1.s; g.ldws = D / 32;
    g.bias = L.b1; g.out = r.big; g.ldo = MLP; g.outs = r.bigs; g.ldos = MLP / 32; g.N = MLP;
  }
  return g;
}

#ifdef CLIPGPU_ABLATE
// Diagnostic build only (make variant VNAME=ablate VDEFS=-DCLIPGPU_ABLATE; tools/ablate.py): skips
// trunk ops so that each op's marginal share of the concurrent-lane step can be measured (the
// numbers are garbage).  Bits: 0 LayerNorm, 1 attention, 2 out_proj, 3 qkv, 4 c_fc, 5 c_proj.
// The product library has no such switch.
unsigned g_ablate = 0;
#define ABLATED(bit) ((g_ablate >> (bit)) & 1u)
extern "C" int clipgpu_test_ablate(unsigned mask) {
  g_ablate = mask;
  return 0;
}
#else
#define ABLATED(bit) false
#endif

namespace {

// Residual rows the head pools from: x at token pos(b) of each sequence (tokens = T), or the
// compact [B][D] rows the pruned last layer leaves (tokens = 1, pos 0).
struct PoolSrc {
  const void* x;  // the residual stream's type (clipgpu_engine::x16)
  int tokens;
  const int64_t* ids;
};

// Last-layer pruning.  The CLIP heads read one token per sequence (CLS, or the EOT argmax
// for text), and after the last layer's attention every op is row-local (out_proj, ln_2,
// c_fc, c_proj), so that layer's tail runs on the pooled rows only: attention still reads
// every token's K/V, then the pooled token's residual row and attention output are gathered
// to a compact [B][D] pair and out_proj .. c_proj run at M = B.  Each kept row goes through
// the same kernels with the same K-ordered sums, so the embeddings are bit-identical to the
// full last layer (test_last_layer_pruning_is_bit_exact).  Off with clipgpu_options.prune_last = -1;
// not for the SigLIP MAP head (pools every token).
// The compact pair lives in the tail of `big`, past the M = B MLP hidden.
inline size_t prune_off_x(const TowerSpec& s, int B) { return align256((size_t)B * mlp_pad(s) * 2); }
inline size_t prune_off_h(const TowerSpec& s, int B) {
  return prune_off_x(s, B) + align256((size_t)B * s.width * 4);
}
inline size_t prune_off_xs(const TowerSpec& s, int B) {  // the compact rows' statistics (ln_fold)
  return prune_off_h(s, B) + align256((size_t)B * s.width * 2);
}
inline bool prune_last(const clipgpu_engine& e, int B, int T) {
  const TowerSpec& s = e.spec;
  return e.prune && s.family != FAMILY_SIGLIP && s.layers > 0 &&
         prune_off_xs(s, B) + ((size_t)B + 256) * 8 <= (size_t)B * T * big_wide(s) * 2;
}

// The transformer trunk shared by both towers: L x [LN1 -> QKV -> MHA -> out+res ->
// LN2 -> fc1+act -> fc2+res], with h already holding ln_1(x) of layer 0.  ids: the text
// tower's token ids (pooled-token choice when the last layer is pruned), nullptr for CLS.
// T: tokens per sequence (the text tower's trimmed length, else the tower's own).
PoolSrc trunk(const clipgpu_engine& e, const Replica& r, int B, int causal, const int64_t* ids, hipStream_t st,
              int T, int pool_pos = 0) {
  const TowerSpec& s = e.spec;
  const int D = s.width;
  const bool prune = prune_last(e, B, T);
  for (int l = 0; l < s.layers; ++l) {
    const LayerW& L = r.w.layers[l];
    const bool compact = prune && l + 1 == s.layers;
    Replica c = r;  // the buffers the tail of this layer runs on
    int rows = B * T;
    auto gemm = [&](int site, int cat, const char* what) {
      if (ABLATED(site == GS_QKV ? 3 : site == GS_OUT ? 2 : site == GS_FC ? 4 : 5)) return;
      ProfScope ps(e, rows == B * T ? cat : PC_TAIL, st, /*gemm=*/true);
      const bool tuned = 2 * rows > e.tuned_rows;
      if (mx_at(e, l, site)) {
        MxGemmParams g = site_gemm_mx(e, c, L, site, rows);
        g.tile = tuned ? e.mxtile[site] : MX_TILE_AUTO;
        check(launch_gemm_mx(e.dt, site_epi_mx(e, l, site), site == GS_FC ? s.act : ACT_NONE, g, st), what);
        return;
      }
      GemmParams g = site_gemm(e, c, L, site, rows);
      g.tile = tuned ? e.tile[site] : TILE_AUTO;
      check(launch_gemm(e.dt, A_ROWS, site_epi(e, site), site == GS_FC ? s.act : ACT_NONE, g, st), what);
    };
    gemm(GS_QKV, PC_QKV, "qkv gemm");
    if (!ABLATED(1)) { ProfScope ps(e, PC_ATTN, st);
      check(launch_attention(e.dt, r.big, r.h, B, T, s.heads, D, causal, st), "attention"); }
    if (compact) {  // pooled rows only from here on (QKV in `big` is dead after attention)
      c.x = (char*)r.big + prune_off_x(s, B);
      c.h = (char*)r.big + prune_off_h(s, B);
      c.xs = (float*)((char*)r.big + prune_off_xs(s, B));
      rows = B;
      ProfScope ps(e, PC_TAIL, st);
      // ids == nullptr: position pool_pos of every sequence (CLS 0, SigLIP2 text T - 1)
      check(launch_gather_pooled(xrows(e, r.x, pool_pos), e.x16, (char*)r.h + (size_t)pool_pos * D * 2, ids, T, c.x, c.h,
                                 B, D, st),
            "gather pooled rows");
    }
    gemm(GS_OUT, PC_OUT_PROJ, "out_proj gemm");
    if (!ABLATED(0)) {
      ProfScope ps(e, compact ? PC_TAIL : PC_LN, st);
      if (e.lnf)  // (folded into c_fc: its rows' statistics only)
        check(launch_ln_stats(c.x, 1, s.ln_eps, c.xs, rows, D, st), "ln_2 statistics");
      else
        check(launch_ln_rows(e.dt, c.x, e.x16, L.ln2_w, L.ln2_b, s.ln_eps, c.h, rows, D, st, ln_q(e, l, GS_FC, c.hs)),
              "ln_2");
    }
    gemm(GS_FC, PC_C_FC, "c_fc gemm");
    gemm(GS_PROJ, PC_C_PROJ, "c_proj gemm");
    if (l + 1 < s.layers && !ABLATED(0)) {
      ProfScope ps(e, PC_LN, st);
      if (e.lnf)  // (folded into the next QKV: its rows' statistics only)
        check(launch_ln_stats(r.x, 1, s.ln_eps, r.xs, rows, D, st), "ln_1 statistics");
      else
        check(launch_ln_rows(e.dt, r.x, e.x16, r.w.layers[l + 1].ln1_w, r.w.layers[l + 1].ln1_b, s.ln_eps, r.h, rows,
                             D, st, ln_q(e, l + 1, GS_QKV, r.hs)),
              "ln_1");
    }
    if (compact) return PoolSrc{c.x, 1, nullptr};
  }
  return PoolSrc{xrows(e, r.x, pool_pos), T, ids};
}

void head(const clipgpu_engine& e, const Replica& r, int B, const PoolSrc& src, float* d_out, hipStream_t st) {
  const TowerSpec& s = e.spec;
  const int D = s.width, E = s.embed_dim;
  ProfScope ps(e, PC_HEAD, st);
  check(launch_pool_ln(e.dt, src.x, e.x16, src.ids, src.tokens, r.w.lnpost_w, r.w.lnpost_b, s.ln_eps, r.pooled, B, D,
                       st),
        "pool+ln");
  check(launch_gemm(e.dt, A_ROWS, EPI_STORE32, ACT_NONE, rows_gemm(r.pooled, D, r.w.proj_t, r.w.proj_b, r.emb, E, B, E, D),
                    st),
        "proj gemm");
  check(launch_l2norm(r.emb, d_out, B, E, st), "l2norm");
}

// SigLIP tail (timm VisionTransformer.norm + AttentionPoolLatent, timm_proj "none"):
// LN(all tokens) -> [k|v] GEMM -> MAP attention with the precomputed latent query -> proj
// -> y + MLP(LN(y)) -> L2 normalise.  Scratch: h (tokens, then the pooled LN), big ([k|v],
// then the MLP hidden), pooled (attention output), x's first B rows (y, f32).
void head_map(const clipgpu_engine& e, const Replica& r, int B, float* d_out, hipStream_t st) {
  const TowerSpec& s = e.spec;
  const int D = s.width, T = s.tokens(), M = mlp_pad(s);
  const MapHeadW& mw = r.w.map;
  ProfScope ps(e, PC_HEAD, st);
  check(launch_ln_rows(e.dt, r.x, 0, r.w.lnpost_w, r.w.lnpost_b, s.ln_eps, r.h, B * T, D, st), "norm");
  check(launch_gemm(e.dt, A_ROWS, EPI_STORE16, ACT_NONE, rows_gemm(r.h, D, mw.wkv, mw.bkv, r.big, 2 * D, B * T, 2 * D, D),
                    st), "attn_pool kv gemm");
  check(launch_map_attention(e.dt, mw.q, r.big, r.pooled, B, T, s.heads, D, st), "attn_pool attention");
  check(launch_gemm(e.dt, A_ROWS, EPI_STORE32, ACT_NONE, rows_gemm(r.pooled, D, mw.wproj, mw.bproj, r.x, D, B, D, D), st),
        "attn_pool proj gemm");
  check(launch_ln_rows(e.dt, r.x, 0, mw.norm_w, mw.norm_b, s.ln_eps, r.h, B, D, st), "attn_pool norm");
  check(launch_gemm(e.dt, A_ROWS, EPI_STORE16, s.act, rows_gemm(r.h, D, mw.w1, mw.b1, r.big, M, B, M, D), st),
        "attn_pool fc1 gemm");
  check(launch_gemm(e.dt, A_ROWS, EPI_RESID, ACT_NONE, rows_gemm(r.big, M, mw.w2, mw.b2, r.x, D, B, D, M), st),
        "attn_pool fc2 gemm");
  check(launch_l2norm((const float*)r.x, d_out, B, D, st), "l2norm");
}

}  // namespace

// conv1 = patch rows (16-bit, staged in `big`) x conv_w^T, epilogue + bias + pos -> x
GemmParams patch_gemm(const clipgpu_engine& e, const Replica& r, int rows) {
  const TowerSpec& s = e.spec;
  const int Kp = kpatch_pad(s);
  GemmParams g = rows_gemm(r.big, Kp, r.w.conv_w, r.w.conv_b, r.x, s.width, rows, s.width, Kp);
  g.G = s.grid();
  g.pos = r.w.pos;
  g.cls = s.cls() ? 1 : 0;
  g.x16 = e.x16 ? 1 : 0;
  return g;
}

// asrc: A_IMG_F32 (pixels = normalised f32 NCHW) or A_IMG_U8 (NHWC u8 + mean/std)
void vision_forward(const clipgpu_engine& e, const Replica& r, const void* pixels, int asrc, const float* mean,
                    const float* stdv, int B, float* d_out, hipStream_t st) {
  const TowerSpec& s = e.spec;
  const int D = s.width, G = s.grid(), P = s.patch_size, Kp = kpatch_pad(s);
  { ProfScope ps(e, PC_PATCH, st);
    check(launch_patch_rows(e.dt, asrc, pixels, mean, stdv, r.big, B, s.image_size, P, kpatch(s), Kp, st),
          "patch rows");
    GemmParams g = patch_gemm(e, r, B * G * G);
    g.tile = 2 * B * s.tokens() > e.tuned_rows ? e.tile_patch : TILE_AUTO;
    check(launch_gemm(e.dt, A_ROWS, EPI_PATCH, ACT_NONE, g, st), "patch gemm"); }
  if (s.family == FAMILY_SIGLIP) {  // no class token, no pre-norm: x = patches + bias + pos
    { ProfScope ps(e, PC_STEM, st);
      check(launch_ln_rows(e.dt, r.x, e.x16, r.w.layers[0].ln1_w, r.w.layers[0].ln1_b, s.ln_eps, r.h, B * s.tokens(), D, st,
                           ln_q(e, 0, GS_QKV, r.hs)),
            "ln_1"); }
    trunk(e, r, B, 0, nullptr, st, s.tokens());
    head_map(e, r, B, d_out, st);
    return;
  }
  {
  ProfScope ps(e, PC_STEM, st);
  check(launch_vision_embed_ln(e.dt, r.x, e.x16, r.w.cls, r.w.pos, r.w.lnpre_w, r.w.lnpre_b, r.w.layers[0].ln1_w,
                               r.w.layers[0].ln1_b, s.ln_eps, e.lnf ? nullptr : r.h, B, s.tokens(), D, st,
                               ln_q(e, 0, GS_QKV, r.hs), r.xs),
        "embed+ln_pre");
  }
  head(e, r, B, trunk(e, r, B, 0, nullptr, st, s.tokens()), d_out, st);
}

// T: tokens per sequence in d_ids ([B][T]): the context length, or a trimmed length (every
// sequence's EOT inside the first T tokens, clipgpu_embed_tokens) -- causal attention makes
// the tokens after a sequence's EOT invisible to its pooled row.
void text_forward(const clipgpu_engine& e, const Replica& r, const int64_t* d_ids, int B, float* d_out,
                  hipStream_t st, int T) {
  const TowerSpec& s = e.spec;
  if (T <= 0) T = s.context_length;
  {
  ProfScope ps(e, PC_STEM, st);
  check(launch_text_embed_ln(e.dt, d_ids, r.w.tok, r.w.pos, r.w.layers[0].ln1_w, r.w.layers[0].ln1_b, s.ln_eps,
                             r.x, e.x16, e.lnf ? nullptr : r.h, B, T, s.width, s.vocab_size, st,
                             ln_q(e, 0, GS_QKV, r.hs), r.xs),
        "token embed+ln_1");
  }
  // CLIP: causal, the EOT (argmax id) row pooled; SigLIP2: no mask, the last position pooled
  head(e, r, B, trunk(e, r, B, s.causal ? 1 : 0, s.pool_last ? nullptr : d_ids, st, T, s.pool_last ? T - 1 : 0),
       d_out, st);
}

// The replica's workspace seen from batch row b0: every activation buffer is
// batch-major, so a sub-batch is a pointer offset.
Replica lane_view(const clipgpu_engine& e, const Replica& r, int b0) {
  const TowerSpec& s = e.spec;
  const size_t rows = (size_t)b0 * s.tokens(), D = s.width;
  const size_t wide = big_wide(s);
  Replica v = r;
  v.x = (char*)r.x + rows * D * xbytes(e);
  v.xs = r.xs + rows * 2;
  v.h = (char*)r.h + rows * D * 2;
  v.big = (char*)r.big + rows * wide * 2;
  if (r.hs) v.hs = r.hs + rows * D / 32;
  if (r.bigs) v.bigs = r.bigs + rows * (size_t)mlp_pad(s) / 32;
  v.pooled = (char*)r.pooled + (size_t)b0 * D * 2;
  v.emb = r.emb + (size_t)b0 * s.embed_dim;
  return v;
}

namespace {

// Batch split for `lanes` concurrent sub-batches: lane i gets rows [b0, b1).
inline void lane_range(int B, int lanes, int i, int& b0, int& b1) {
  b0 = (int)((long)B * i / lanes);
  b1 = (int)((long)B * (i + 1) / lanes);
}

inline int lanes_for(const clipgpu_engine& e, int B) {
  return B < 8 * e.dev_lanes ? 1 : e.dev_lanes;  // small batches gain nothing from lanes
}

// Runs fwd(view, b0, n, stream) on each lane, forked from and joined back to `st`.
// While profiling, the same per-lane launches run one after another on `st`, so
// each kernel's HIP-event time is its own (same shapes as the concurrent run).
template <typename F>
void run_lanes(const clipgpu_engine& e, const Replica& r, int B, hipStream_t st, F fwd) {
  const int L = lanes_for(e, B);
  // profiling serializes the lanes (each event pair times one kernel alone), unless the mask asks
  // for the concurrent regime (CLIPGPU_PROFILE_CONCURRENT)
  const bool serial = e.prof.mask != 0 && !(e.prof.mask & CLIPGPU_PROFILE_CONCURRENT);
  if (L == 1 || serial) {
    for (int i = 0; i < L; ++i) {
      int b0, b1;
      lane_range(B, L, i, b0, b1);
      fwd(lane_view(e, r, b0), b0, b1 - b0, st);
    }
    return;
  }
  HIP_CHECK(hipEventRecord(r.fork, st));
  for (int i = 0; i < L; ++i) {
    int b0, b1;
    lane_range(B, L, i, b0, b1);
    HIP_CHECK(hipStreamWaitEvent(r.lane[i], r.fork, 0));
    fwd(lane_view(e, r, b0), b0, b1 - b0, r.lane[i]);
    HIP_CHECK(hipEventRecord(r.join[i], r.lane[i]));
  }
  for (int i = 0; i < L; ++i) HIP_CHECK(hipStreamWaitEvent(st, r.join[i], 0));
}

}  // namespace

void vision_forward_lanes(const clipgpu_engine& e, const Replica& r, const void* pixels, int asrc, const float* mean,
                          const float* stdv, int B, float* d_out, hipStream_t st) {
  const size_t S = e.spec.image_size;
  const size_t row_bytes = 3 * S * S * (asrc == A_IMG_F32 ? 4 : 1);
  const int E = e.spec.embed_dim;
  run_lanes(e, r, B, st, [&](const Replica& v, int b0, int n, hipStream_t ls) {
    vision_forward(e, v, (const char*)pixels + b0 * row_bytes, asrc, mean, stdv, n, d_out + (size_t)b0 * E, ls);
  });
}

void text_forward_lanes(const clipgpu_engine& e, const Replica& r, const int64_t* d_ids, int B, float* d_out,
                        hipStream_t st) {
  const int E = e.spec.embed_dim, T = e.spec.context_length;
  run_lanes(e, r, B, st, [&](const Replica& v, int b0, int n, hipStream_t ls) {
    text_forward(e, v, d_ids + (size_t)b0 * T, n, d_out + (size_t)b0 * E, ls);
  });
}

}  // namespace clipgpu
