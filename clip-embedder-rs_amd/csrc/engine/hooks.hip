// Test hooks that read or set a handle's state (include/clipgpu_testing.h), the profiler API and
// clipgpu_synth_tensor.
#include "engine.hpp"

namespace clipgpu {

namespace {
static const char* kProfNames[PC_N] = {"patch_embed", "stem_ln", "qkv", "attention", "out_proj",
                                       "layernorm", "c_fc", "c_proj", "head", "last_layer"};
}  // namespace

}  // namespace clipgpu

using namespace clipgpu;

extern "C" {

int clipgpu_test_read_weights(const char* model_dir, int tower, const char* name, float* out, int64_t n) {
  return guarded([&]() {
    if (!model_dir || !name || !out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    if (tower != CLIPGPU_TOWER_VISION && tower != CLIPGPU_TOWER_TEXT) throw ClipErr(CLIPGPU_ERR_INVALID, "bad tower");
    const std::string dir(model_dir);
    TensorMap m;
    try {
      const OpenClipConfig oc = load_open_clip_config(dir + "/open_clip_config.json");
      m = load_tower_weights(dir, tower == CLIPGPU_TOWER_VISION ? oc.vision : oc.text);
    } catch (const std::runtime_error& ex) {
      throw ClipErr(CLIPGPU_ERR_CONFIG, ex.what());
    }
    auto it = m.find(name);
    if (it == m.end()) throw ClipErr(CLIPGPU_ERR_INVALID, std::string("no parameter ") + name);
    if (it->second.numel() != n) throw ClipErr(CLIPGPU_ERR_INVALID, "size mismatch for " + std::string(name));
    std::memcpy(out, it->second.data.data(), (size_t)n * sizeof(float));
  });
}

int clipgpu_test_engine_tiles(const clipgpu_engine* e, int tiles[4]) {
  return guarded([&]() {
    if (!e || !tiles) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) tiles[i] = reported_tile(*e, i);
  });
}

int clipgpu_test_force_broadcast(clipgpu_engine* e, int on) {
  return guarded([&]() {
    if (!e) throw ClipErr(CLIPGPU_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    e->force_bcast = on != 0;
  });
}

// A handle without a communicator takes the multi-device handle's lazy path: its own clique over its
// replicas' (distinct) devices, created by ensure_comm on the first gathered call.
int clipgpu_test_comm_lazy(clipgpu_engine* e) {
  return guarded([&]() {
    if (!e) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL handle");
    if (e->comm_nranks > 0) throw ClipErr(CLIPGPU_ERR_INVALID, "the handle already has a communicator");
    std::vector<int> devs;
    for (auto& r : e->reps) {
      for (int d : devs)
        if (d == r.device) throw ClipErr(CLIPGPU_ERR_INVALID, "a device listed twice has no clique");
      devs.push_back(r.device);
    }
    e->comm_devs = devs;
    e->comm_pending = true;
    e->comm_nranks = (int)devs.size();
    e->comm_rank0 = 0;
  });
}

int clipgpu_test_host_plan(clipgpu_engine* e, int n_chunks, const int* bounds, int copy_stream) {
  return guarded([&]() {
    if (!e) throw ClipErr(CLIPGPU_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    // (copy_stream: the schedule variants of rounds 3-5 were removed in round 6; 0 and 1 both mean the one
    // schedule run_host_shard has)
    if (copy_stream != 0 && copy_stream != 1) throw ClipErr(CLIPGPU_ERR_INVALID, "copy_stream: 0 or 1");
    e->host_part.clear();
    if (n_chunks == 0) return;
    if (n_chunks < 1 || n_chunks > 4 || !bounds) throw ClipErr(CLIPGPU_ERR_INVALID, "1..4 chunks");
    std::vector<int> part{0};
    for (int i = 0; i < n_chunks - 1; ++i) {
      if (bounds[i] <= part.back() || bounds[i] >= e->max_batch)
        throw ClipErr(CLIPGPU_ERR_INVALID, "chunk bounds must increase inside (0, max_batch)");
      part.push_back(bounds[i]);
    }
    part.push_back(e->max_batch);
    e->host_part = part;
  });
}

int clipgpu_test_rgb8_resize_always(clipgpu_engine* e, int on) {
  return guarded([&]() {
    if (!e) throw ClipErr(CLIPGPU_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    e->rgb8_resize_always = on != 0;
  });
}

int clipgpu_test_engine_lanes(const clipgpu_engine* e, int* dev_lanes) {
  return guarded([&]() {
    if (!e || !dev_lanes) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    *dev_lanes = e->dev_lanes;
  });
}

int clipgpu_test_engine_residual(const clipgpu_engine* e, int* residual, int* ln_fold) {
  return guarded([&]() {
    if (!e || !residual) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    *residual = e->x16 ? CLIPGPU_RESIDUAL_F16 : CLIPGPU_RESIDUAL_F32;
    if (ln_fold) *ln_fold = e->lnf ? 1 : 0;
  });
}

int clipgpu_profile_enable(clipgpu_engine* e, unsigned mask) {
  return guarded([&]() {
    if (!e) throw ClipErr(CLIPGPU_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    Profiler& p = e->prof;
    for (auto& rec : p.pending) { (void)hipEventSynchronize(rec.b); }
    p.pending.clear();
    p.used = 0;
    for (int i = 0; i < PC_N; ++i) { p.total_ms[i] = 0; p.count[i] = 0; }
    p.mask = mask;
  });
}

int clipgpu_profile_read(clipgpu_engine* e, int category, double* total_ms, int64_t* launches) {
  return guarded([&]() {
    if (!e || category < 0 || category >= PC_N) throw ClipErr(CLIPGPU_ERR_INVALID, "bad profile query");
    std::lock_guard<std::mutex> lk(e->mu);
    Profiler& p = e->prof;
    for (auto& rec : p.pending) {
      HIP_CHECK(hipEventSynchronize(rec.b));
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, rec.a, rec.b));
      p.total_ms[rec.cat] += ms;
      p.count[rec.cat] += 1;
    }
    p.pending.clear();
    p.used = 0;
    if (total_ms) *total_ms = p.total_ms[category];
    if (launches) *launches = p.count[category];
  });
}

// The recorded launches as a timeline (tools/timeline.py): start / end of each in ms from the first
// recorded start, its category and lane (index of the lane stream it ran on, -1 for another stream).
// Consumes the records like clipgpu_profile_read (which then sees them in its totals).
int clipgpu_test_profile_timeline(clipgpu_engine* e, int64_t n_max, double* t0, double* t1, int* cat, int* lane,
                                  int64_t* n_out) {
  return guarded([&]() {
    if (!e || !n_out || n_max < 0 || (n_max > 0 && (!t0 || !t1 || !cat || !lane)))
      throw ClipErr(CLIPGPU_ERR_INVALID, "bad timeline query");
    std::lock_guard<std::mutex> lk(e->mu);
    Profiler& p = e->prof;
    int64_t n = 0;
    for (auto& rec : p.pending) HIP_CHECK(hipEventSynchronize(rec.b));
    for (auto& rec : p.pending) {
      float ms = 0.f, s0 = 0.f, s1 = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, rec.a, rec.b));
      p.total_ms[rec.cat] += ms;
      p.count[rec.cat] += 1;
      if (n < n_max) {
        HIP_CHECK(hipEventElapsedTime(&s0, p.pending[0].a, rec.a));
        HIP_CHECK(hipEventElapsedTime(&s1, p.pending[0].a, rec.b));
        t0[n] = s0;
        t1[n] = s1;
        cat[n] = rec.cat;
        int ln = -1;
        for (int i = 0; i < 4 && !e->reps.empty(); ++i)
          if (rec.st != nullptr && rec.st == e->reps[0].lane[i]) ln = i;
        lane[n] = ln;
      }
      ++n;
    }
    p.pending.clear();
    p.used = 0;
    *n_out = n;
  });
}

const char* clipgpu_profile_category_name(int category) {
  return (category >= 0 && category < PC_N) ? kProfNames[category] : "";
}

int clipgpu_synth_tensor(uint64_t seed, const char* name, double std_, double offset, float* out, int64_t n) {
  return guarded([&]() {
    if (!name || !out || n < 0) throw ClipErr(CLIPGPU_ERR_INVALID, "bad arguments");
    synth_fill(seed, name, std_, offset, out, n);
  });
}

}  // extern "C"
