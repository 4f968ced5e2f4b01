// clipgpu engine: one tower (vision or text) replicated on one or more GPUs.
//
// Replaces the ONNX Runtime session (src/onnx.rs:7-47) that the reference builds
// per tower and runs in VisionEmbedder::embed_images (src/vision.rs:100-117) and
// TextEmbedder::embed_texts (src/text.rs:148-169).  Weights are uploaded once per
// device (16-bit matrices for MFMA, f32 for LayerNorm/bias/embeddings) into one
// arena; activations live in a persistent per-device workspace sized for
// max_batch, so a forward performs no allocation and can be captured in a
// hipGraph.  Multi-device handles shard the batch into contiguous row blocks,
// one host worker thread and one stream per device.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <vector>

#include "../../../include/clipgpu.h"
#include "../../../include/clipgpu_testing.h"
#include "../bounce.hpp"
#include "../hip_check.hpp"
#include "../host/api_util.hpp"
#include "../host/copy_pool.hpp"
#include "../host/json.hpp"
#include "../host/model.hpp"
#include "../host/resize_plan.hpp"
#include "../kernels/common.hpp"
#include "../kernels/kernels.hpp"

// This header: the structs the pieces of csrc/engine/ share, the small shape helpers and the
// declarations of the functions that cross files (DESIGN.md "Source layout").

namespace clipgpu {

// MX-fp8 weight matrix (fp8 engines): e4m3 [N][K] + E8M0 scales [N][K/32] (gemm_mx.hip).
struct MxW {
  uint8_t* q = nullptr;
  uint8_t* s = nullptr;
};

struct LayerW {
  float *ln1_w, *ln1_b, *bqkv, *bo, *ln2_w, *ln2_b, *b1, *b2;
  // LayerNorm-folded engines (clipgpu_engine::lnf): wqkv / w1 hold W' = f16(W diag(gamma)), bqkv / b1
  // hold b + W beta, and these the column sums of W' (EPI_LNF)
  float *cs_qkv = nullptr, *cs_1 = nullptr;
  void *wqkv, *wo, *w1, *w2;  // 16-bit (fp8 engines: wo only)
  MxW mqkv, m1, m2;           // fp8 engines: QKV, c_fc, c_proj
};

// MAP attention-pool head of the SigLIP family (timm AttentionPoolLatent).
struct MapHeadW {
  float* q = nullptr;                 // [D] f32: latent . Wq^T + bq (the same for every image)
  void *wkv = nullptr, *wproj = nullptr, *w1 = nullptr, *w2 = nullptr;  // 16-bit [N][K]
  float *bkv = nullptr, *bproj = nullptr, *norm_w = nullptr, *norm_b = nullptr, *b1 = nullptr, *b2 = nullptr;
};

struct DevWeights {
  void* conv_w = nullptr;  // [D][Kpad] 16-bit (K = 3*P*P zero-padded to a multiple of 64)
  float* conv_b = nullptr; // SigLIP patch-embedding bias (nullptr for CLIP)
  MapHeadW map;
  float *cls = nullptr, *pos = nullptr, *lnpre_w = nullptr, *lnpre_b = nullptr;
  float* tok = nullptr;  // text token table [V][D] f32
  std::vector<LayerW> layers;
  float *lnpost_w = nullptr, *lnpost_b = nullptr;
  void* proj_t = nullptr;  // [E][D] 16-bit (transposed visual.proj / text_projection)
  float* proj_b = nullptr; // [E] text_projection.bias (SigLIP2 text; nullptr otherwise)
};

// One set of the host path's staging buffers and events (run_host_shard).  Set 0 is filled by
// alloc_workspace, its device rows carved from the work arena; a call of more than max_batch rows
// alternates rounds between two sets, so round i + 1's host copy and H2D run under round i's forward:
// set 1 is allocated on the first such call (ensure_host_set2) and owns its device rows.
struct HostSet {
  void* in = nullptr;        // device input staging (pixels f32 / u8 / ids)
  void* pin_in = nullptr;    // pinned host staging
  float* pin_out = nullptr;
  float* out = nullptr;      // [B][E] f32 device embedding rows
  hipEvent_t done[4] = {nullptr, nullptr, nullptr, nullptr};    // chunk slot's D2H finished
  hipEvent_t copied[4] = {nullptr, nullptr, nullptr, nullptr};  // chunk slot's H2D finished
  bool owns_device = false;  // in / out are allocations of their own (set 1), freed at teardown
};

struct Replica {
  int device = 0;
  hipStream_t stream = nullptr;
  char* arena = nullptr;  // weights
  char* work = nullptr;   // activations
  DevWeights w;
  void* x = nullptr;      // [rows][D] residual stream: f32, or f16 (clipgpu_engine::x16)
  float* xs = nullptr;    // [rows + 256][2] (mean, rstd) of x's rows (LayerNorm-folded engines: ln_stats)
  void* h = nullptr;      // [rows][D] 16-bit (LN output / attention output); fp8 engines: LN output as e4m3
  uint8_t* hs = nullptr;   // fp8 engines: [rows][D/32] scales of the LN output in h
  uint8_t* bigs = nullptr; // fp8 engines: [rows][MLP/32] scales of the c_fc output (e4m3 in big)
  void* big = nullptr;    // [rows][max(3D, MLP)] 16-bit (qkv / MLP hidden)
  void* pooled = nullptr; // [B][D] 16-bit
  float* emb = nullptr;   // [B][E] f32 (pre-normalisation)
  HostSet hset[2];        // host path: input / output staging
  // Concurrent sub-batches ("lanes"): each lane runs the whole forward on a
  // contiguous slice of the batch on its own stream, so one lane's GEMM tail
  // rounds and memory-bound kernels overlap the other lane's GEMMs.
  hipStream_t lane[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t fork = nullptr, join[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t copy = nullptr, copy2 = nullptr;  // host path: every H2D, in chunk order; copy2: multi-round D2Hs
  // Decoded-image path (clipgpu_embed_images_rgb8): per slot, pinned staging and a device
  // arena of [descriptors | ints | raw RGB8 images], and the resize intermediate.  Grown
  // on demand (images have any size); reused across calls.
  struct ImageSlot {
    char* pin = nullptr;
    size_t pin_cap = 0;
    char* dev = nullptr;
    size_t dev_cap = 0;
    uint8_t* tmp = nullptr;
    size_t tmp_cap = 0;
  } islot[4];
  // Captured forwards (hipGraph), keyed by entry point, buffers and batch; owned here,
  // shared by the lane views.
  struct GraphCache* graphs = nullptr;
  hipEvent_t gin = nullptr, gout = nullptr;  // fork / join around a graph launched for a caller stream
  // RCCL communicator of this replica's rank (the one collective, an all-gather of
  // the embedding rows over xGMI): ncclCommInitAll over a multi-device handle's devices, or
  // ncclCommInitRank for one-process-per-GPU deployments (clipgpu_comm_init_rank).
  ncclComm_t comm = nullptr;
  hipEvent_t coll = nullptr;  // recorded behind this replica's last collective (destroy_comms waits for it)
};

// Replayable forwards: one hipGraphExec per (entry point, input / output buffers, batch,
// normalisation constants).  A forward is ~90 dependent launches per lane; replaying it
// as one graph removes the per-launch host cost and most inter-kernel dispatch gaps.
// Bounded: at kMax entries the least recently replayed one is destroyed, after every stream of
// the replica (the capture stream and the lane streams a host-path slot replays on) has drained,
// since any of them may still be running it.
struct GraphCache {
  struct Entry {
    std::vector<uint64_t> key;
    hipGraphExec_t exec;
    uint64_t last_use;
  };
  std::vector<Entry> entries;
  uint64_t clock = 0;
  static constexpr size_t kMax = 32;
  void clear() {
    for (auto& en : entries) (void)hipGraphExecDestroy(en.exec);
    entries.clear();
  }
};

// Live per-kernel-class timing with HIP events recorded on the launch stream
// (clipgpu_profile_*; bench.py's roofline.achieved).  Off by default.
enum ProfCat { PC_PATCH = 0, PC_STEM, PC_QKV, PC_ATTN, PC_OUT_PROJ, PC_LN, PC_C_FC, PC_C_PROJ, PC_HEAD, PC_TAIL, PC_N };
struct Profiler {
  unsigned mask = 0;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  struct Rec { int cat; hipEvent_t a, b; hipStream_t st; };
  std::vector<Rec> pending;
  double total_ms[PC_N] = {0};
  long long count[PC_N] = {0};
  hipEvent_t get() {
    if (used == pool.size()) {
      hipEvent_t ev;
      if (hipEventCreate(&ev) != hipSuccess) return nullptr;
      pool.push_back(ev);
    }
    return pool[used++];
  }
};

}  // namespace clipgpu

struct clipgpu_engine {
  clipgpu::Profiler prof;
  // GEMM tile per trunk call site (clipgpu::GemmSite), autotuned at creation for
  // max_batch rows; batches under half of that use the shape heuristic.
  int tile[4] = {0, 0, 0, 0};
  int mxtile[4] = {0, 0, 0, 0};  // fp8 engines: MxTile of the MX sites (tile[] then holds the 16-bit tile
                                 // the site runs on layers outside mx_layers)
  int tile_patch = 0;  // vision: the patch-embedding GEMM (tuned with the trunk sites)
  int tuned_rows = 0;
  int lanes = 1;  // lane streams / host-path slots per device (clipgpu_options.lanes, default 2)
  // Concurrent sub-batches of a device-side forward: the tile table's choice, or `lanes` when
  // clipgpu_options.lanes pins it (full-batch GEMMs quantize better over the CUs than two
  // half-batch ones; the lanes overlap LayerNorm / attention with GEMMs).
  int dev_lanes = 1;
  bool lanes_pinned = false;
  bool graphs = true;  // replay forwards as hipGraphs (clipgpu_options.graphs = -1 disables)
  bool prune = true;   // last layer on the pooled rows only (clipgpu_options.prune_last = -1 disables; trunk)
  bool trim = true;    // host-ids text batches run on their first max(EOT)+1 tokens (options.trim_text = -1: off)
  // The residual stream x is stored in f16 (clipgpu_options.residual): its two read-modify-writes and
  // two LayerNorm reads per layer move half the bytes; every add into it and every LayerNorm statistic
  // stays f32.  bf16 / f16 engines of the CLIP family only (fp8 engines' MX residual epilogue and the
  // SigLIP MAP head take the f32 stream).
  bool x16 = false;
  // ln_1 / ln_2 folded into the QKV / c_fc GEMMs (clipgpu_options.ln_fold; f16 stream only): those
  // GEMMs read x (f16) with W' = W diag(gamma) (f16) and EPI_LNF; no LayerNorm launches in the trunk.
  bool lnf = false;

  int tuning = 0;  // clipgpu_options.tuning: 1 = timing tuner (+ whole-forward pass), 2 = per-site pass only
  // clipgpu_options.gemm_tiles / patch_tile pins (0 = the table's tile, -1 = the shape heuristic)
  int pin_tiles[4] = {0, 0, 0, 0};
  int pin_patch = 0;
  // fp8 engines: layer l runs its MX sites in MX-fp8 iff bit l is set (clipgpu_options.mx_layers; 0 =
  // every layer); the other layers run bf16 at every site
  uint64_t mx_layers = ~0ull;
  // Multi-device handles over distinct devices: the RCCL communicator is created on the first
  // gathered call (comm_pending), or at creation when clipgpu_options.communicator = 1.
  bool comm_pending = false;
  std::vector<int> comm_devs;
  bool force_bcast = false;  // test hook: gathered calls take the ragged (broadcast) branch
  // test hook (clipgpu_test_host_plan): the host path's chunk partition of max_batch (empty = host_chunks'
  // default)
  std::vector<int> host_part;
  // test hook (clipgpu_test_rgb8_resize_always): S x S decoded images also take the resize path
  bool rgb8_resize_always = false;
  clipgpu::TowerSpec spec;
  clipgpu::PreprocessCfg pre;
  clipgpu::DType dt = clipgpu::DT_BF16;
  // fp8 engine (CLIPGPU_DTYPE_FP8): QKV / c_fc / c_proj run as MX-fp8 GEMMs (e4m3 weights +
  // activations, E8M0 block scales, v_mfma_scale_f32_32x32x64_f8f6f4); attention, out_proj,
  // the stems and heads stay bf16.
  bool mx = false;
  // The MX sites of an fp8 engine (clipgpu_options.mx_sites, a subset of qkv / fc / proj; c_proj in MX
  // needs c_fc in MX, whose epilogue quantizes the hidden activations).  Default: all three.
  bool mx_site[4] = {false, false, false, false};  // indexed by GemmSite (GS_OUT stays bf16)
  int max_batch = 0;
  size_t in_bytes_per_row = 0;
  std::vector<clipgpu::Replica> reps;
  // Communicator geometry: comm_nranks ranks in all; replica i is rank comm_rank0 + i.
  int comm_nranks = 0, comm_rank0 = 0;
  std::mutex mu;  // one call per handle at a time (src/vision.rs:107 write lock)
};

// The helpers and cross-file functions below are the engine's own: none of them is exported.
#pragma GCC visibility push(hidden)
namespace clipgpu {

enum GemmSite { GS_QKV = 0, GS_OUT, GS_FC, GS_PROJ, GS_N };

// fp8 engines: does layer l run `site` as an MX-fp8 GEMM (the engine's MX sites, on the layers of
// clipgpu_options.mx_layers)?
inline bool mx_at(const clipgpu_engine& e, int l, int site) {
  return e.mx_site[site] && l >= 0 && l < 64 && ((e.mx_layers >> l) & 1ull);
}

inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
inline int round64(int n) { return (n + 63) / 64 * 64; }
// GEMM K / N dims are multiples of 64: the MLP hidden width and the patch-embedding
// K = 3*P*P are zero-padded (exact: padded c_fc rows / bias are 0 and act(0) = 0 for
// every supported activation; padded conv columns multiply zero-filled pixels).
inline int mlp_pad(const TowerSpec& s) { return round64(s.mlp_width); }
inline int kpatch(const TowerSpec& s) { return 3 * s.patch_size * s.patch_size; }
inline int kpatch_pad(const TowerSpec& s) { return round64(kpatch(s)); }
// Elements per token row of the `big` scratch: QKV (3D), the MLP hidden width, and for
// the vision tower also the staged patch rows (G^2 rows of kpatch_pad per image, which
// the patch GEMM consumes before layer 0 writes QKV).
inline size_t big_wide(const TowerSpec& s) {
  size_t w = std::max((size_t)3 * s.width, (size_t)mlp_pad(s));
  if (s.tower == TOWER_VISION) {
    const size_t G = (size_t)s.image_size / s.patch_size, T = (size_t)s.tokens();
    w = std::max(w, (G * G * (size_t)kpatch_pad(s) + T - 1) / T);
  }
  return w;
}

// The residual stream's element size and row offsets (f32, or f16: clipgpu_engine::x16).
inline size_t xbytes(const clipgpu_engine& e) { return e.x16 ? 2 : 4; }
inline void* xrows(const clipgpu_engine& e, void* x, size_t rows) {
  return (char*)x + rows * (size_t)e.spec.width * xbytes(e);
}

enum InKind { IN_F32 = 0, IN_U8 = 1, IN_IDS = 2 };

// Row source of a host entry point: a contiguous array (row i at in + i * row_bytes), or one pointer per
// row (`rows`: the decoded-image entry point's S x S images, which already are the u8 NHWC rows).
struct HostRows {
  const char* in = nullptr;
  const void* const* rows = nullptr;
  size_t row_bytes = 0;
};

inline uint64_t fbits(const float* v, int i) {
  uint32_t u = 0;
  if (v) std::memcpy(&u, v + i, 4);
  return u;
}

inline void need_tower(const clipgpu_engine* e, int tower) {
  if (!e) throw ClipErr(CLIPGPU_ERR_INVALID, "engine is NULL");
  if (e->spec.tower != tower)
    throw ClipErr(CLIPGPU_ERR_INVALID, tower == TOWER_VISION ? "engine is not a vision tower" : "engine is not a text tower");
}

// The tile a trunk site reports (clipgpu_engine_info, clipgpu_test_engine_tiles): the MxTile of an MX site.
inline int reported_tile(const clipgpu_engine& e, int site) { return e.mx_site[site] ? e.mxtile[site] : e.tile[site]; }

// weights.hip
void upload_weights(clipgpu_engine& e, Replica& r, const TensorMap& m);
void alloc_workspace(clipgpu_engine& e, Replica& r);
void destroy_replica(Replica& r);

// forward.hip
struct SiteShape { int N, K; };
SiteShape site_shape(const clipgpu_engine& e, int site);  // a trunk site's GEMM is rows x N x K
int site_epi(const clipgpu_engine& e, int site);
int site_epi_mx(const clipgpu_engine& e, int l, int site);
GemmParams site_gemm(const clipgpu_engine& e, const Replica& r, const LayerW& L, int site, int rows);
MxGemmParams site_gemm_mx(const clipgpu_engine& e, const Replica& r, const LayerW& L, int site, int rows);
GemmParams patch_gemm(const clipgpu_engine& e, const Replica& r, int rows);  // rows = images x G^2 patch rows
void vision_forward(const clipgpu_engine& e, const Replica& r, const void* pixels, int asrc, const float* mean,
                    const float* stdv, int B, float* d_out, hipStream_t st);
void text_forward(const clipgpu_engine& e, const Replica& r, const int64_t* d_ids, int B, float* d_out,
                  hipStream_t st, int T = 0);
Replica lane_view(const clipgpu_engine& e, const Replica& r, int b0);
void vision_forward_lanes(const clipgpu_engine& e, const Replica& r, const void* pixels, int asrc, const float* mean,
                          const float* stdv, int B, float* d_out, hipStream_t st);
void text_forward_lanes(const clipgpu_engine& e, const Replica& r, const int64_t* d_ids, int B, float* d_out,
                        hipStream_t st);
#ifdef CLIPGPU_ABLATE
extern unsigned g_ablate;  // diagnostic build only (forward.hip): part of run_graph's key
#endif

// tiles.hip
void table_tiles(clipgpu_engine& e);
void apply_tile_pins(clipgpu_engine& e);
void autotune_tiles(clipgpu_engine& e, Replica& r);
void tune_forward(clipgpu_engine& e, Replica& r);

// gather.hip
void ensure_comm(clipgpu_engine& e);
void destroy_comms(clipgpu_engine& e);

// Runs body(stream) as a replayed hipGraph (captured on first use of `key`).  The capture
// and replay stream is `st` when it is one of the replica's own streams, else the replica's
// stream, forked from and joined back to `st` by events (a caller's stream may be the
// legacy null stream, which cannot be captured).  Profiling (per-launch events) and
// clipgpu_options.graphs = -1 run the body directly.
template <typename F>
void run_graph(const clipgpu_engine& e, const Replica& r, const std::vector<uint64_t>& key_in, hipStream_t st, F body) {
  if (!e.graphs || e.prof.mask || !r.graphs) {
    body(st);
    return;
  }
  bool own = st == r.stream;
  for (int i = 0; i < 4; ++i) own = own || (st != nullptr && st == r.lane[i]);
  hipStream_t gs = own ? st : r.stream;
  GraphCache& gc = *r.graphs;
  hipGraphExec_t exec = nullptr;
#ifdef CLIPGPU_ABLATE
  std::vector<uint64_t> key = key_in;
  key.push_back(0xAB1A7E00u | g_ablate);
#else
  const std::vector<uint64_t>& key = key_in;
#endif
  ++gc.clock;
  for (auto& en : gc.entries)
    if (en.key == key) {
      exec = en.exec;
      en.last_use = gc.clock;
    }
  if (!exec && gc.entries.size() >= GraphCache::kMax) {  // evict the least recently used graph
    HIP_CHECK(hipStreamSynchronize(r.stream));
    for (int i = 0; i < 4; ++i)
      if (r.lane[i]) HIP_CHECK(hipStreamSynchronize(r.lane[i]));
    if (!own) HIP_CHECK(hipStreamSynchronize(st));
    size_t lru = 0;
    for (size_t i = 1; i < gc.entries.size(); ++i)
      if (gc.entries[i].last_use < gc.entries[lru].last_use) lru = i;
    (void)hipGraphExecDestroy(gc.entries[lru].exec);
    gc.entries.erase(gc.entries.begin() + (long)lru);
  }
  if (!own) {
    HIP_CHECK(hipEventRecord(r.gin, st));
    HIP_CHECK(hipStreamWaitEvent(gs, r.gin, 0));
  }
  if (!exec) {
    hipGraph_t g = nullptr;
    HIP_CHECK(hipStreamBeginCapture(gs, hipStreamCaptureModeRelaxed));
    try {
      body(gs);
    } catch (...) {
      (void)hipStreamEndCapture(gs, &g);
      if (g) (void)hipGraphDestroy(g);
      throw;
    }
    HIP_CHECK(hipStreamEndCapture(gs, &g));
    const hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIP_CHECK(ie);
    gc.entries.push_back({key, exec, gc.clock});
  }
  HIP_CHECK(hipGraphLaunch(exec, gs));
  if (!own) {
    HIP_CHECK(hipEventRecord(r.gout, gs));
    HIP_CHECK(hipStreamWaitEvent(st, r.gout, 0));
  }
}

}  // namespace clipgpu
#pragma GCC visibility pop
