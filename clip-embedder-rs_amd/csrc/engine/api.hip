// The public C API (include/clipgpu.h) of the engine: creation and teardown of a handle, the getters,
// the device-buffer entry points and the similarity entry points.
#include "engine.hpp"

namespace clipgpu {

namespace {

// Everything a handle holds: comms first, then per replica its device's memory, streams, events and
// graphs (destroy_replica).  clipgpu_destroy runs it, and so does every failed clipgpu_create_ex, on
// whatever had been built by then.
void destroy_engine(clipgpu_engine* e) {
  for (hipEvent_t ev : e->prof.pool) (void)hipEventDestroy(ev);
  destroy_comms(*e);
  for (auto& r : e->reps) destroy_replica(r);
  delete e;
}

// The *_device entry points' prologue: the tower, the batch (and `null_arg`: the message of a NULL
// argument found by the caller, checked after the batch), then the handle's lock -- one enqueue per handle
// at a time (graph cache, workspace) -- and its device.
std::unique_lock<std::mutex> device_call(clipgpu_engine* e, int tower, int64_t B, const char* null_arg = nullptr) {
  need_tower(e, tower);
  if (B <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (B > e->max_batch) throw ClipErr(CLIPGPU_ERR_INVALID, "B exceeds max_batch");
  if (null_arg) throw ClipErr(CLIPGPU_ERR_INVALID, null_arg);
  std::unique_lock<std::mutex> lk(e->mu);
  HIP_CHECK(hipSetDevice(e->reps[0].device));
  return lk;
}

bool file_exists(const std::string& p) {
  struct stat st;
  return ::stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

// clipgpu_options.residual = 0: the residual stream's default storage
constexpr int kResidualDefault = CLIPGPU_RESIDUAL_F16;

}  // namespace

}  // namespace clipgpu

using namespace clipgpu;

extern "C" {

int clipgpu_abi_version(void) { return CLIPGPU_ABI_VERSION; }

int clipgpu_options_init(clipgpu_options* o) {
  return guarded([&]() {
    if (!o) throw ClipErr(CLIPGPU_ERR_INVALID, "opts is NULL");
    std::memset(o, 0, sizeof(*o));
    o->struct_size = sizeof(*o);
  });
}

int clipgpu_create(const char* model_dir, int tower, const int* device_ids, int n_devices, int dtype, int max_batch,
                   clipgpu_engine** out) {
  return clipgpu_create_ex(model_dir, tower, device_ids, n_devices, dtype, max_batch, nullptr, out);
}

int clipgpu_create_ex(const char* model_dir, int tower, const int* device_ids, int n_devices, int dtype,
                      int max_batch, const clipgpu_options* opts_in, clipgpu_engine** out) {
  return guarded([&]() {
    if (!out) throw ClipErr(CLIPGPU_ERR_INVALID, "out is NULL");
    *out = nullptr;
    clipgpu_options opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.struct_size = sizeof(opts);
    if (opts_in) {  // an older caller's smaller struct: its prefix, defaults for the rest
      // the sizes of the struct's published versions only: v2 (through `communicator`), v3 (through
      // `mx_layers`) and v4 (a size ending inside a field would copy part of it)
      if (opts_in->struct_size != offsetof(clipgpu_options, graphs) &&
          opts_in->struct_size != offsetof(clipgpu_options, residual) && opts_in->struct_size != sizeof(opts))
        throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.struct_size: call clipgpu_options_init first");
      std::memcpy(&opts, opts_in, opts_in->struct_size);
    }
    if (opts.mx_sites & ~(CLIPGPU_MX_QKV | CLIPGPU_MX_FC | CLIPGPU_MX_PROJ))
      throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.mx_sites: unknown bits");
    if (opts.lanes < 0 || opts.lanes > 4) throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.lanes must be 0..4");
    if (opts.tuning < 0 || opts.tuning > 2) throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.tuning must be 0, 1 or 2");
    for (int32_t v : {opts.graphs, opts.prune_last, opts.trim_text})
      if (v < -1 || v > 1) throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options graphs / prune_last / trim_text: -1, 0 or 1");
    for (int i = 0; i < 5; ++i) {
      const int t = i < 4 ? opts.gemm_tiles[i] : opts.patch_tile;
      if (t != 0 && t != -1 && !gemm_tile_built(t))
        throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.gemm_tiles / patch_tile: " + std::to_string(t) +
                                               " is not a GEMM tile this library builds");
    }
    if (opts.mx_layers != 0 && dtype != CLIPGPU_DTYPE_FP8)
      throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.mx_layers needs dtype CLIPGPU_DTYPE_FP8");
    if (opts.residual < 0 || opts.residual > CLIPGPU_RESIDUAL_F16)
      throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.residual must be 0, 1 (f32) or 2 (f16)");
    if (opts.ln_fold < -1 || opts.ln_fold > 1)
      throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.ln_fold must be -1, 0 or 1");
    if (opts.communicator < 0 || opts.communicator > 1)
      throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.communicator must be 0 or 1");
    if (!model_dir) throw ClipErr(CLIPGPU_ERR_INVALID, "model_dir is NULL");
    if (tower != CLIPGPU_TOWER_VISION && tower != CLIPGPU_TOWER_TEXT) throw ClipErr(CLIPGPU_ERR_INVALID, "bad tower");
    if (dtype != CLIPGPU_DTYPE_BF16 && dtype != CLIPGPU_DTYPE_F16 && dtype != CLIPGPU_DTYPE_FP8)
      throw ClipErr(CLIPGPU_ERR_INVALID, "bad dtype");
    if (max_batch <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "max_batch must be > 0");
    const std::string dir(model_dir);
    struct stat st;
    if (::stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode))
      throw ClipErr(CLIPGPU_ERR_CONFIG, "Model folder not found: '" + dir + "'");  // ClipError::ModelFolderNotFound
    for (const char* f : {"open_clip_config.json", "model_config.json"})
      if (!file_exists(dir + "/" + f))
        throw ClipErr(CLIPGPU_ERR_CONFIG, std::string("Missing model file '") + f + "' in folder '" + dir + "'");
    OpenClipConfig oc;
    try {
      oc = load_open_clip_config(dir + "/open_clip_config.json");
    } catch (const std::runtime_error& ex) {
      throw ClipErr(CLIPGPU_ERR_CONFIG, ex.what());
    }
    std::unique_ptr<clipgpu_engine, void (*)(clipgpu_engine*)> e(new clipgpu_engine(), destroy_engine);
    e->spec = tower == CLIPGPU_TOWER_VISION ? oc.vision : oc.text;
    e->pre = oc.pre;
    e->dt = dtype == CLIPGPU_DTYPE_F16 ? DT_F16 : DT_BF16;  // fp8 engines keep bf16 outside the MX GEMMs
    e->mx = dtype == CLIPGPU_DTYPE_FP8;
    if (e->mx) {  // the MX split: the options' bits, else all three sites
      const uint32_t bits = opts.mx_sites ? opts.mx_sites : (CLIPGPU_MX_QKV | CLIPGPU_MX_FC | CLIPGPU_MX_PROJ);
      e->mx_site[GS_QKV] = (bits & CLIPGPU_MX_QKV) != 0;
      e->mx_site[GS_FC] = (bits & CLIPGPU_MX_FC) != 0;
      e->mx_site[GS_PROJ] = (bits & CLIPGPU_MX_PROJ) != 0;
      if (e->mx_site[GS_PROJ] && !e->mx_site[GS_FC])
        throw ClipErr(CLIPGPU_ERR_INVALID, "MX sites: proj in MX needs fc in MX");
      if (e->spec.layers < 32 && (opts.mx_layers >> e->spec.layers) != 0)
        throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.mx_layers: bit set at or beyond the tower's " +
                                               std::to_string(e->spec.layers) + " layers");
      e->mx_layers = opts.mx_layers ? (uint64_t)opts.mx_layers : ~0ull;
    } else if (opts.mx_sites) {
      throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.mx_sites needs dtype CLIPGPU_DTYPE_FP8");
    }
    e->max_batch = max_batch;
    if (opts.lanes > 0) {
      e->lanes = opts.lanes;
      e->lanes_pinned = true;
    } else {
      e->lanes = 2;  // host-path staging slots (run_host_shard); the device-side lane count is the table's
    }
    e->tuning = opts.tuning;
    e->dev_lanes = e->lanes;
    e->graphs = opts.graphs != -1;
    e->prune = opts.prune_last != -1;
    e->trim = opts.trim_text != -1;
    {  // the residual stream's storage (clipgpu_options.residual; kResidualDefault when 0)
      const int res = opts.residual ? opts.residual : kResidualDefault;
      const bool f16_ok = e->spec.family != FAMILY_SIGLIP;
      if (opts.residual == CLIPGPU_RESIDUAL_F16 && !f16_ok)
        throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_options.residual = f16: CLIP-family engines only");
      e->x16 = res == CLIPGPU_RESIDUAL_F16 && f16_ok;
      // the LayerNorm fold (clipgpu_options.ln_fold): the f16 stream, a QuickGELU / GELU MLP
      const bool fold_ok = e->x16 && !e->mx && (e->spec.act == ACT_QUICK_GELU || e->spec.act == ACT_GELU);
      if (opts.ln_fold == 1 && !fold_ok)
        throw ClipErr(CLIPGPU_ERR_INVALID,
                      "clipgpu_options.ln_fold = 1: needs a bf16 / f16 engine, the f16 residual stream and a "
                      "QuickGELU / GELU MLP");
      e->lnf = fold_ok && opts.ln_fold != -1;
    }
    for (int i = 0; i < 4; ++i) e->pin_tiles[i] = opts.gemm_tiles[i];
    e->pin_patch = opts.patch_tile;
    const TowerSpec& s = e->spec;
    if (!s.unsupported.empty()) throw ClipErr(CLIPGPU_ERR_CONFIG, s.unsupported);
    if (s.heads <= 0 || s.width % s.heads || s.width % 64)
      throw ClipErr(CLIPGPU_ERR_CONFIG, "Configuration error: width must be a multiple of 64 and of heads");
    const int hd = s.width / s.heads;
    if (hd != 64 && hd != 72 && hd != 80)
      throw ClipErr(CLIPGPU_ERR_CONFIG, "Configuration error: head dim " + std::to_string(hd) + " not supported (64, 72, 80)");
    if (s.width > 1280) throw ClipErr(CLIPGPU_ERR_CONFIG, "Configuration error: width > 1280 not supported yet");
    if (e->mx && (s.width % 128 || mlp_pad(s) % 128))
      throw ClipErr(CLIPGPU_ERR_CONFIG, "Configuration error: the fp8 path needs width and MLP width % 128 == 0");
    if (s.tokens() > 1024) throw ClipErr(CLIPGPU_ERR_CONFIG, "Configuration error: > 1024 tokens not supported yet");
    if (s.tower == TOWER_VISION) {
      if (s.image_size % s.patch_size)
        throw ClipErr(CLIPGPU_ERR_CONFIG, "Configuration error: image_size must be a multiple of patch_size");
      e->in_bytes_per_row = (size_t)3 * s.image_size * s.image_size * 4;  // f32 (u8 path uses a quarter)
    } else {
      e->in_bytes_per_row = (size_t)s.context_length * 8;
    }
    // weights
    TensorMap m;
    try {
      m = load_tower_weights(dir, s);
    } catch (const std::runtime_error& ex) {
      throw ClipErr(CLIPGPU_ERR_CONFIG, ex.what());
    }
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    std::vector<int> devs;
    if (device_ids && n_devices > 0) devs.assign(device_ids, device_ids + n_devices);
    else devs.push_back(0);
    for (int d : devs)
      if (d < 0 || d >= ndev) throw ClipErr(CLIPGPU_ERR_DEVICE, "device id " + std::to_string(d) + " not available");
    e->reps.resize(devs.size());
    for (size_t i = 0; i < devs.size(); ++i) {
      Replica& r = e->reps[i];
      r.device = devs[i];
      HIP_CHECK(hipSetDevice(r.device));
      HIP_CHECK(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
      upload_weights(*e, r, m);
      alloc_workspace(*e, r);
      if (i == 0) {  // one tile choice, shared by identical devices
        if (e->tuning) {
          autotune_tiles(*e, r);
          apply_tile_pins(*e);
          tune_forward(*e, r);
        } else {
          table_tiles(*e);
          apply_tile_pins(*e);
        }
      }
    }
    // A multi-device handle over distinct devices gets one communicator (ncclCommInitAll; rank i
    // = device_ids[i]; RCCL refuses two ranks on one GPU, so a handle that lists a device twice
    // keeps the host-buffer sharding and has no collective entry points).  It is created on the
    // first gathered call (ensure_comm) unless the options ask for it now: creation and the
    // host-buffer entry points never depend on RCCL.  A one-device handle gets a one-rank clique
    // through the same code when clipgpu_options.communicator = 1 asks for one (else it joins a
    // deployment's communicator with clipgpu_comm_init_rank).
    bool distinct = devs.size() > 1 || (devs.size() == 1 && opts.communicator == 1);
    for (size_t i = 0; i < devs.size() && distinct; ++i)
      for (size_t j = i + 1; j < devs.size(); ++j) distinct = distinct && devs[i] != devs[j];
    if (distinct) {
      e->comm_devs = devs;
      e->comm_pending = true;
      e->comm_nranks = (int)devs.size();
      e->comm_rank0 = 0;
      if (opts.communicator == 1) ensure_comm(*e);
    }
    *out = e.release();
  });
}

void clipgpu_destroy(clipgpu_engine* e) {
  if (e) destroy_engine(e);
}

int clipgpu_embed_dim(const clipgpu_engine* e) { return e ? e->spec.embed_dim : -1; }
int clipgpu_input_size(const clipgpu_engine* e) {
  return e ? (e->spec.tower == TOWER_VISION ? e->spec.image_size : e->spec.context_length) : -1;
}
int clipgpu_num_devices(const clipgpu_engine* e) { return e ? (int)e->reps.size() : -1; }

int clipgpu_embed_pixels_device(clipgpu_engine* e, const float* d_nchw, int64_t B, float* d_out, void* stream) {
  return guarded([&]() {
    const auto lk = device_call(e, TOWER_VISION, B);
    Replica& r = e->reps[0];
    run_graph(*e, r, {1, (uint64_t)d_nchw, (uint64_t)d_out, (uint64_t)B}, (hipStream_t)stream,
              [&](hipStream_t gs) { vision_forward_lanes(*e, r, d_nchw, A_IMG_F32, nullptr, nullptr, (int)B, d_out, gs); });
  });
}

int clipgpu_embed_u8_device(clipgpu_engine* e, const uint8_t* d_nhwc, int64_t B, const float mean[3],
                            const float stdv[3], float* d_out, void* stream) {
  return guarded([&]() {
    const auto lk = device_call(e, TOWER_VISION, B, !mean || !stdv ? "NULL mean/std" : nullptr);
    Replica& r = e->reps[0];
    run_graph(*e, r,
              {2, (uint64_t)d_nhwc, (uint64_t)d_out, (uint64_t)B, fbits(mean, 0), fbits(mean, 1), fbits(mean, 2),
               fbits(stdv, 0), fbits(stdv, 1), fbits(stdv, 2)},
              (hipStream_t)stream,
              [&](hipStream_t gs) { vision_forward_lanes(*e, r, d_nhwc, A_IMG_U8, mean, stdv, (int)B, d_out, gs); });
  });
}

static void check_similarity_args(int64_t n_img, int64_t n_txt, int64_t E, int activation, int axis) {
  if (n_img <= 0 || n_txt <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (E <= 0 || E % 16) throw ClipErr(CLIPGPU_ERR_INVALID, "Shape error: embedding dim must be a multiple of 16");
  // 65535 * 64: launch_similarity's grid has one y block per 64 image rows
  if (n_img > 65535L * 64 || n_txt > (1L << 30) || n_img * n_txt > (1L << 40))
    throw ClipErr(CLIPGPU_ERR_INVALID, "Shape error: similarity matrix too large");
  if (activation < CLIPGPU_SIM_SOFTMAX || activation > CLIPGPU_SIM_LOGITS || axis < 0 || axis > 1)
    throw ClipErr(CLIPGPU_ERR_INVALID, "bad activation / axis");
}

int clipgpu_similarity_device(const float* d_img, int64_t n_img, const float* d_txt, int64_t n_txt, int64_t E,
                              float logit_scale, float logit_bias, int activation, int axis, float* d_out,
                              void* stream) {
  return guarded([&]() {
    check_similarity_args(n_img, n_txt, E, activation, axis);
    if (!d_img || !d_txt || !d_out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    check(launch_similarity(d_img, (int)n_img, d_txt, (int)n_txt, (int)E, logit_scale, logit_bias, activation, axis,
                            d_out, (hipStream_t)stream),
          "similarity");
  });
}

int clipgpu_similarity(int device, const float* img, int64_t n_img, const float* txt, int64_t n_txt, int64_t E,
                       float logit_scale, float logit_bias, int activation, int axis, float* out) {
  return guarded([&]() {
    check_similarity_args(n_img, n_txt, E, activation, axis);
    if (!img || !txt || !out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    HIP_CHECK(hipSetDevice(device));
    const size_t bi = (size_t)n_img * E * 4, bt = (size_t)n_txt * E * 4, bo = (size_t)n_img * n_txt * 4;
    char* d = nullptr;
    HIP_CHECK(hipMalloc((void**)&d, align256(bi) + align256(bt) + bo));
    float *di = (float*)d, *dt = (float*)(d + align256(bi)), *dO = (float*)(d + align256(bi) + align256(bt));
    hipError_t err = copy_h2d(di, img, bi);
    if (err == hipSuccess) err = copy_h2d(dt, txt, bt);
    if (err == hipSuccess)
      err = launch_similarity(di, (int)n_img, dt, (int)n_txt, (int)E, logit_scale, logit_bias, activation, axis, dO,
                              nullptr);
    if (err == hipSuccess) err = copy_d2h(out, dO, bo);
    (void)hipFree(d);
    check(err, "similarity");
  });
}

int clipgpu_embed_tokens_device(clipgpu_engine* e, const int64_t* d_ids, int64_t B, float* d_out, void* stream) {
  return guarded([&]() {
    const auto lk = device_call(e, TOWER_TEXT, B);
    Replica& r = e->reps[0];
    run_graph(*e, r, {3, (uint64_t)d_ids, (uint64_t)d_out, (uint64_t)B}, (hipStream_t)stream,
              [&](hipStream_t gs) { text_forward_lanes(*e, r, d_ids, (int)B, d_out, gs); });
  });
}

int clipgpu_engine_info(const clipgpu_engine* e, int tiles[4], int* lanes, uint32_t* mx_sites) {
  return guarded([&]() {
    if (!e) throw ClipErr(CLIPGPU_ERR_INVALID, "engine is NULL");
    if (tiles)
      for (int i = 0; i < 4; ++i) tiles[i] = reported_tile(*e, i);
    if (lanes) *lanes = e->dev_lanes;
    if (mx_sites)
      *mx_sites = (e->mx_site[GS_QKV] ? CLIPGPU_MX_QKV : 0u) | (e->mx_site[GS_FC] ? CLIPGPU_MX_FC : 0u) |
                  (e->mx_site[GS_PROJ] ? CLIPGPU_MX_PROJ : 0u);
  });
}

}  // extern "C"
