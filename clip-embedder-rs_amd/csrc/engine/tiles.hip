// Which GEMM tile each trunk site runs and how many lanes a device-side forward takes: the committed
// MI355X table (the default) and the two timing tuners.
#include "engine.hpp"

namespace clipgpu {

namespace {

// The committed MI355X tile table (default; clipgpu_options.tuning = 0).  A trunk site's tile is
// a function of its GEMM shape at the rows one lane runs at max_batch, so an engine's kernels --
// and the profiles and PMC records taken of them -- are the same on every box and every run.  The
// entries are the timing tuner's (below) majority choice over repeated runs on MI355X
// (tools/tile_table.py, profiles/r03_v13_tile_table.jsonl); the tile choice never changes the output
// bits (every tile computes the same K-ordered sums, test_gemm_tile_choice_is_bit_exact).
//   qkv / c_fc (N = 3D / MLP wide, K = D): 256x256 with the half-tile last round (tile 18, which
//     falls back to plain 256x256 RS where the half round does not apply);
//   out_proj / c_proj (N = D, + residual): 160x128 8-wave RS (tile 17), two blocks per CU; except
//     the wide, K-long c_proj of ViT-H/14 (N >= 1280, K >= 5120): 192x256 8-wave (tile 13), 681-685
//     vs 725-740 us at 46720 x 1280 x 5120 in two interleaved A/B sessions
//     (profiles/r03_v2_gemm_ab_pp.txt, r03_v7_tile_256x128_half_ab.txt); at every other N = D shape
//     of the BASELINE models tile 17 is the fastest or within 1 %;
//   rows < 2048 (small max_batch): the shape heuristic (TILE_AUTO; skinny kernel <= 256 rows).
// `rows` is one lane's rows at max_batch; the lane count is table_lanes' (below), and the two-lane
// ViT-B/32 regime overrides out_proj / c_fc / c_proj / patch in table_tiles.
int table_tile(const clipgpu_engine& e, int site, int rows) {
  if (rows < 2048) return TILE_AUTO;
  const int N = site_shape(e, site).N, K = site_shape(e, site).K;
  switch (site) {
    case GS_QKV: return TILE_256x256_HALF;
    case GS_FC: return TILE_256x256_HALF;
    default: return N >= 1280 && K >= 5120 ? TILE_192x256_W8 : TILE_160x128_W8_RS;
  }
}

// Device lanes of the committed table.  A large-batch text tower (>= 32768 token rows: configs[2]'s
// 1024 x 77) takes two lanes: its LayerNorms and causal attention are a larger
// share of the layer than in the vision trunk (0.7 + 0.7 ms of 9.3 ms at one lane) and overlap the
// other lane's GEMMs, while 39424-row lanes still fill the 256x256 / 160x128 rounds (round 2's
// two-lane text leg: 117k seq/s; round 3's one-lane table: 110k; profiles/r03_v12_text_lanes_ab.txt).
// Round 4: a vision batch of 8192..32767 token rows (ViT-B/32 at 256 images: 12800) takes two
// lanes too, with out_proj, c_fc, c_proj and the patch GEMM off the 8-wave 160x128 tile (table_tiles
// below: c_fc on the 4-wave 160x128 RS tile, two blocks per CU, one from each lane).  Same-box A/Bs (tools/bench_variants.sh,
// profiles/r04_lanes_ab.jsonl): one lane on the 8-wave table tiles 79.8-80.3k img/s; two lanes on the
// same tiles 81.3k; two lanes with these 82.6-84.2k (qkv on 256x256 plain, RS or half-tile within
// 0.5 %; c_fc on 256x256 at two lanes loses 2 %).  The round-1 tree -- two lanes of 160x128 tiles
// -- ran 83.4k on the same box as this tree's one-lane table's 79.8k (profiles/r04_ab_trees.jsonl):
// round 3's move to one lane was the 80.9k of BENCH_r03.
constexpr long kVisionTwoLaneRows[2] = {8192, 32768};
bool vision_two_lanes(const clipgpu_engine& e) {
  const long rows = (long)e.max_batch * e.spec.tokens();
  return e.spec.tower == TOWER_VISION && rows >= kVisionTwoLaneRows[0] && rows < kVisionTwoLaneRows[1];
}
// Larger vision batches take two lanes on their one-lane tiles: DFN5B ViT-H/14-378 at 64 images
// (46720 rows) 862 -> 886 img/s, SO400M-16-SigLIP2-384 at 128 (73728 rows) 1545 -> 1545
// (tools/bench_models.py lanesab, profiles/r04_large_model_lanes_ab.jsonl, two rounds each).
int table_lanes(const clipgpu_engine& e) {
  const long rows = (long)e.max_batch * e.spec.tokens();
  if (e.spec.tower == TOWER_VISION) return rows >= kVisionTwoLaneRows[0] ? 2 : 1;
  return e.spec.tower == TOWER_TEXT && rows >= 32768 ? 2 : 1;
}

}  // namespace

void table_tiles(clipgpu_engine& e) {
  if (!e.lanes_pinned) e.dev_lanes = table_lanes(e);
  const int rows = (e.max_batch + e.dev_lanes - 1) / e.dev_lanes * e.spec.tokens();
  e.tuned_rows = rows;
  for (int site = 0; site < GS_N; ++site) {
    e.tile[site] = table_tile(e, site, rows);
    e.mxtile[site] = MX_TILE_AUTO;
  }
  // Large text batches: c_proj (N = 512, K = 2048) on the 4-wave 160x128 RS tile, two blocks per CU
  // beside the other lane's work: 113.2-113.7k -> 116.6-116.8k seq/s in a same-box A/B against
  // the 8-wave tile 17 (profiles/r03_v13_text_tiles_ab.txt; the tuner's pick was 15 as well)
  // (measured for the two-lane regime only, so tied to it)
  if (e.spec.tower == TOWER_TEXT && e.dev_lanes == 2 && rows >= 16384) e.tile[GS_PROJ] = TILE_160x128_RS;
  // the patch-embedding GEMM has the c_proj shape class (N = D, K = 3 P^2 padded)
  const int G = e.spec.grid();
  const int prow = e.spec.tower == TOWER_VISION ? rows / e.spec.tokens() * G * G : 0;
  e.tile_patch = prow >= 2048 ? TILE_160x128_W8_RS : TILE_AUTO;
  // the two-lane vision regime (table_lanes): qkv, c_fc, c_proj and the patch GEMM (c_proj's shape class)
  // on the 4-wave 160x128 RS tile (two blocks per CU), out_proj on the 8-wave 224x192 tile (one round of
  // 116 tiles per 6400-row lane).  qkv moved off the 256x256 half tile in round 6: the same 26 us alone,
  // 94.2k vs 92.9k img/s in the forward (profiles/r06_qkv_tile_ab.txt).  Round 4 put c_proj on 224x192 too (+0.4-0.9 %, f32 stream,
  // profiles/r04_residual26_two_lanes_ab.jsonl); with the f16 stream and the round-6 DMA issue,
  // c_proj alone takes 41.4 us on 160x128 against 57.1 us on 224x192 and the step is as fast or faster
  // (93.1k vs 92.3k img/s, profiles/r06_residual_tiles_ab.txt); c_fc on 224x192 loses 3 %
  if (vision_two_lanes(e) && e.dev_lanes == 2 && rows >= 2048) {
    e.tile[GS_QKV] = e.tile[GS_FC] = e.tile[GS_PROJ] = TILE_160x128_RS;
    e.tile[GS_OUT] = TILE_224x192_W8;
    if (prow >= 2048) e.tile_patch = TILE_160x128_RS;
    if (e.mx) {  // fp8 engines: the timing tuner's picks in this regime, 105.0k vs 102.6k img/s over the MX
                 // shape heuristic (profiles/r06_fp8_tiles_probe.jsonl)
      e.mxtile[GS_QKV] = MX_TILE_256x128;
      e.mxtile[GS_FC] = e.mxtile[GS_PROJ] = MX_TILE_128x128;
      e.tile[GS_OUT] = TILE_160x128_RS;
    }
  }
}

// clipgpu_options.gemm_tiles / patch_tile pins over the table's (or the tuner's) choice: a GemmTile
// id, or -1 = the shape heuristic (TILE_AUTO).  Validated at creation (built tiles only).
void apply_tile_pins(clipgpu_engine& e) {
  for (int i = 0; i < GS_N; ++i)
    if (e.pin_tiles[i]) e.tile[i] = e.pin_tiles[i] < 0 ? TILE_AUTO : e.pin_tiles[i];
  if (e.pin_patch) e.tile_patch = e.pin_patch < 0 ? TILE_AUTO : e.pin_patch;
}

namespace {

bool tiles_pinned(const clipgpu_engine& e) {
  bool any = e.pin_patch != 0;
  for (int t : e.pin_tiles) any = any || t != 0;
  return any;
}

// The tiles both timing passes choose from (the per-site autotune and tune_forward's coordinate
// descent): every tile the library builds (kGemmTiles).
const auto& kTuneCands = kGemmTiles;
constexpr int kMxTuneCands[] = {MX_TILE_256x128, MX_TILE_128x128};  // the built MX tiles

// The tuners' clock: a pair of events on one stream.
struct Stopwatch {
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  explicit Stopwatch(hipStream_t s) : st(s) {}
  ~Stopwatch() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  // ms of `iters` runs of run() (which enqueues its work on the stream), after one untimed run
  template <typename F>
  float time(int iters, F run) {
    if (!a) HIP_CHECK(hipEventCreate(&a));
    if (!b) HIP_CHECK(hipEventCreate(&b));
    run();
    HIP_CHECK(hipEventRecord(a, st));
    for (int i = 0; i < iters; ++i) run();
    HIP_CHECK(hipEventRecord(b, st));
    HIP_CHECK(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return ms;
  }
  // The fastest of `cands` (`fallback` if none is timed); launch(tile) enqueues the candidate once.
  template <typename C, typename F>
  int fastest(const C& cands, int fallback, F launch) {
    float best = 1e30f;
    for (int t : cands) {
      const float ms = time(4, [&]() { launch(t); });
      if (ms < best) {
        best = ms;
        fallback = t;
      }
    }
    return fallback;
  }
};

}  // namespace

// Timing tuner (clipgpu_options.tuning = 1 / 2; tools/tile_table.py uses it to regenerate the table):
// times each candidate tile on every trunk GEMM site at max_batch rows (workspace contents are
// scratch at this point) and keeps the fastest.  Tile choice changes speed only: every tile computes
// the same sums in the same K order.
void autotune_tiles(clipgpu_engine& e, Replica& r) {
  // tuned for the rows one lane runs at max_batch
  const int rows = (e.max_batch + e.dev_lanes - 1) / e.dev_lanes * e.spec.tokens();
  e.tuned_rows = rows;
  Stopwatch sw(r.stream);
  auto tune = [&](GemmParams g, int epi, int act) {
    return sw.fastest(kTuneCands, TILE_AUTO, [&](int t) {
      g.tile = t;
      check(launch_gemm(e.dt, A_ROWS, epi, act, g, r.stream), "autotune gemm");
    });
  };
  const LayerW& L = r.w.layers[0];
  for (int site = 0; site < GS_N; ++site) {
    const int act = site == GS_FC ? e.spec.act : ACT_NONE;
    if (mx_at(e, 0, site)) {  // MX sites: the built MX tiles
      MxGemmParams g = site_gemm_mx(e, r, L, site, rows);
      e.mxtile[site] = sw.fastest(kMxTuneCands, e.mxtile[site], [&](int t) {
        g.tile = t;
        check(launch_gemm_mx(e.dt, site_epi_mx(e, 0, site), act, g, r.stream), "autotune mx gemm");
      });
    }
    if (e.mx && (e.mx_layers & 1ull) && e.mx_site[site]) {
      // a 16-bit GEMM runs at this site only on layers outside mx_layers: the table's tile there
      e.tile[site] = table_tile(e, site, rows);
      continue;
    }
    e.tile[site] = tune(site_gemm(e, r, L, site, rows), site_epi(e, site), act);
  }
  // (the patch GEMM of the images one lane runs)
  if (e.spec.tower == TOWER_VISION)
    e.tile_patch = tune(patch_gemm(e, r, rows / e.spec.tokens() * e.spec.grid() * e.spec.grid()), EPI_PATCH, ACT_NONE);
}


// Second tuning pass over whole forwards: the per-site autotune times each GEMM alone, but
// in the forward two lanes' kernels share the chip, so a tile that wins alone can lose there.
// Coordinate descent: for each trunk site, try every other tile with the rest fixed and keep
// it if the concurrent-lane forward at max_batch gets >= 1 % faster.  Inputs are the zeroed
// staging buffer (timing only).  clipgpu_options.tuning = 2 skips it; pinned tiles skip it.
void tune_forward(clipgpu_engine& e, Replica& r) {
  if (e.tuning != 1 || tiles_pinned(e) || e.max_batch < 64 || e.mx) return;
  const int B = e.max_batch;
  Stopwatch sw(r.stream);
  const HostSet& hs = r.hset[0];
  auto fwd = [&]() {
    if (e.spec.tower == TOWER_VISION)
      vision_forward_lanes(e, r, hs.in, A_IMG_F32, nullptr, nullptr, B, hs.out, r.stream);
    else
      text_forward_lanes(e, r, (const int64_t*)hs.in, B, hs.out, r.stream);
  };
  // the better of two timings: one disturbed measurement does not decide a choice
  auto time_fwd = [&]() {
    const float first = sw.time(3, fwd);
    return std::min(first, sw.time(3, fwd));
  };
  float best = time_fwd();
  if (!e.lanes_pinned && e.lanes > 1) {  // lanes: the configured count, or the whole batch on one stream
    int keep_tiles[GS_N], keep_patch = e.tile_patch, keep_rows = e.tuned_rows;
    for (int i = 0; i < GS_N; ++i) keep_tiles[i] = e.tile[i];
    e.dev_lanes = 1;
    autotune_tiles(e, r);
    const float one = time_fwd();
    if (one < 0.99f * best) {
      best = one;
    } else {  // back to the lanes and their tiles
      e.dev_lanes = e.lanes;
      for (int i = 0; i < GS_N; ++i) e.tile[i] = keep_tiles[i];
      e.tile_patch = keep_patch;
      e.tuned_rows = keep_rows;
    }
  }
  for (int site = 0; site < GS_N; ++site) {
    const int keep = e.tile[site];
    for (int t : kTuneCands) {
      if (t == keep) continue;
      const int prev = e.tile[site];
      e.tile[site] = t;
      const float ms = time_fwd();
      if (ms < 0.99f * best) {  // confirm against the kept tile re-timed before and after the
        e.tile[site] = prev;    // candidate's second timing: neither a lucky timing nor a clock
        const float kept = time_fwd();  // drift between timings decides the choice
        e.tile[site] = t;
        const float again = time_fwd();
        e.tile[site] = prev;
        const float kept2 = time_fwd();
        if (again < 0.99f * std::min(kept, kept2)) {
          e.tile[site] = t;
          best = std::min(ms, again);
        } else {
          best = std::min(best, std::min(kept, kept2));
        }
      } else {
        e.tile[site] = prev;
      }
    }
  }
}

}  // namespace clipgpu
