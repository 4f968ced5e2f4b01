// The embedding index of include/clipgpu.h: a gallery of embeddings that stays on one GPU between
// calls, searched by the fused top-k kernels (kernels/topk.hip) -- what the reference's users do
// with the embeddings (README.md:76-82, examples/search.rs, Clip::rank_images src/clip.rs:134-170)
// without the [queries][gallery] score matrix or a host sort.
//
// Everything is allocated at creation: the gallery at its fixed capacity and one work area (the
// search workspace + staging for the host-buffer search's query chunk and results).  A mutex
// serialises the callers of a handle; on the device, each operation waits for the event recorded
// after the previous one, so an add on one stream followed by a search on another is ordered and
// two searches never share the workspace at once.
//
// Removal and filters.  The authoritative live bitmap is on the host (allocated at the first remove; none
// = every row live) and mirrored to the work area.  A search with removed rows or an allow bitmap first
// writes eff = live & allow into the work area (once per call) and runs the masked kernels on it; any
// other search runs the unmasked kernels as before.
//
// Probabilities (clipgpu_index_search_probs).  The same search with one more output, the softmax over the
// searched rows or the sigmoid of the k results.  The softmax needs one (max, sum) pair per (query row,
// span); they live in the work area too (64 pairs per phase-1 block the workspace holds), as do the host
// form's staged probabilities and (max, sum) rows.  The other searches run the kernels they ran before.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/clipgpu.h"
#include "bounce.hpp"
#include "hip_check.hpp"
#include "host/api_util.hpp"
#include "kernels/kernels.hpp"

using namespace clipgpu;

namespace {

constexpr int64_t kQueryChunk = 256;  // queries per launch: 4 query tiles
constexpr int kMaxBlocks = 1024;      // phase-1 blocks per launch the workspace is sized for (4 per CU)
inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

struct clipgpu_index {
  std::mutex mu;
  int device = 0;
  int64_t E = 0, capacity = 0, size = 0;
  int dtype = CLIPGPU_INDEX_F32;  // the gallery's element type
  int64_t esz = 4;                // its bytes
  char* gallery = nullptr;        // [capacity][E] of esz bytes
  char* work = nullptr;      // ws | staged queries | staged indices | staged scores | live | eff | pairs | staged probs | staged norms
  int ws_blocks = 0;         // phase-1 blocks the workspace holds: min(kMaxBlocks, 4 * 64-row tiles of capacity)
  float* st_q = nullptr;
  int64_t* st_idx = nullptr;
  float* st_score = nullptr;
  uint32_t* d_live = nullptr;    // the mirror of h_live; bits at and past `size` are ones; read only while n_dead > 0
  uint32_t* d_eff = nullptr;     // the filter of the search in flight: live & allow, whole 64-row tiles
  void* d_ms = nullptr;          // the softmax search in flight: one (max, sum) per (query row, span), 64 * ws_blocks
  float* st_prob = nullptr;
  float* st_norm = nullptr;
  std::vector<uint32_t> h_live;  // bit i: row i is live; ceil(capacity / 32) words, empty = every row live
  int64_t n_dead = 0;            // cleared bits of h_live below `size`
  float* scratch = nullptr;      // 16-bit index: f32 rows on their way in (add) or out (get_rows); lazy
  size_t scratch_bytes = 0;
  hipStream_t stream = nullptr;  // the host-buffer forms' stream
  hipEvent_t done = nullptr;     // recorded after every device-side operation
};

namespace {

void order_after_last(clipgpu_index* ix, hipStream_t s) { HIP_CHECK(hipStreamWaitEvent(s, ix->done, 0)); }
void mark_last(clipgpu_index* ix, hipStream_t s) { HIP_CHECK(hipEventRecord(ix->done, s)); }

void check_add(const clipgpu_index* ix, const float* rows, int64_t n) {
  if (!ix || !rows) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (n <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
}

void check_search(const clipgpu_index* ix, const float* q, int64_t nq, int64_t k, const int64_t* idx,
                  const float* score) {
  if (!ix || !q || !idx || !score) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (nq <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (k < 1 || k > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k must be in 1.." + std::to_string(CLIPGPU_TOPK_MAX) +
                                           " (clipgpu_similarity gives the whole matrix)");
}

int64_t live_words(int64_t rows) { return (rows + 31) / 32; }
bool is_live(const clipgpu_index* ix, int64_t i) { return ix->h_live.empty() || ((ix->h_live[i >> 5] >> (i & 31)) & 1u); }

// The filter of one search call, written on `s` (which the caller has ordered after the handle's last
// operation): NULL if nothing filters (no allow bitmap, no removed row), else d_eff = live & allow.
// d_allow: device words (d_eff itself for the host form, which stages its bitmap there) or NULL.
const uint32_t* build_mask(clipgpu_index* ix, const uint32_t* d_allow, hipStream_t s) {
  if (!d_allow && ix->n_dead == 0) return nullptr;
  HIP_CHECK(launch_topk_mask(ix->n_dead ? ix->d_live : nullptr, d_allow, ix->d_eff, ix->size, s));
  return ix->d_eff;
}

// Searches d_q [nq][E] in chunks of kQueryChunk rows on `s`, all under one mask.  probs: TOPK_PROBS_NONE, or
// the probabilities too (d_prob [nq][k]; d_norm [nq][2] or NULL, softmax only).  The span cut is the same with
// and without them: a launch of B phase-1 blocks writes at most 64 B pairs (wide: 64 rows per block; few-query:
// 16 rows and at most 4 * ws_blocks spans), which the pair area holds.
void search_on(clipgpu_index* ix, const float* d_q, int64_t nq, int64_t k, float scale, float bias,
               const uint32_t* mask, int64_t* d_idx, float* d_score, hipStream_t s, int probs = TOPK_PROBS_NONE,
               float* d_prob = nullptr, float* d_norm = nullptr) {
  for (int64_t q0 = 0; q0 < nq; q0 += kQueryChunk) {
    const int rows = (int)std::min(kQueryChunk, nq - q0);
    const TopkPlan p = topk_plan(ix->size, rows, ix->ws_blocks);  // the route too: few rows, few-query kernel
    const TopkProbs pr = {probs, ix->d_ms, 64L * ix->ws_blocks, d_prob ? d_prob + q0 * k : nullptr,
                          d_norm ? d_norm + q0 * 2 : nullptr};
    HIP_CHECK(launch_topk(d_q + q0 * ix->E, rows, ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, scale, bias,
                         (int)k, p, ix->work, mask, d_idx + q0 * k, d_score + q0 * k, s,
                         probs == TOPK_PROBS_NONE ? nullptr : &pr));
  }
  mark_last(ix, s);
}

// The activation of a probability search as the kernels name it; refused before any device call.
int probs_kind(int activation) {
  if (activation == CLIPGPU_SIM_SOFTMAX) return TOPK_PROBS_SOFTMAX;
  if (activation == CLIPGPU_SIM_SIGMOID) return TOPK_PROBS_SIGMOID;
  throw ClipErr(CLIPGPU_ERR_INVALID, "activation must be CLIPGPU_SIM_SOFTMAX or CLIPGPU_SIM_SIGMOID "
                                     "(logits: clipgpu_index_search_filtered)");
}

// The live words that hold rows [0, size) to the device mirror (synchronous).  Callers hold the mutex
// and have waited for `done`.
void upload_live(clipgpu_index* ix) {
  HIP_CHECK(copy_h2d(ix->d_live, ix->h_live.data(), (size_t)live_words(ix->size) * 4));
}

void check_ids(const clipgpu_index* ix, const int64_t* ids, int64_t n) {
  if (!ix || (!ids && n > 0)) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (n < 0) throw ClipErr(CLIPGPU_ERR_INVALID, "negative count");
}
void check_ids_in_range(const clipgpu_index* ix, const int64_t* ids, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= ix->size) throw ClipErr(CLIPGPU_ERR_INVALID, "id out of range (0 <= id < size)");
}

// Device scratch for the f32 side of a 16-bit index's host-row add / export, in pieces of at most 64 MiB
// (one row if a row is larger).  The handle keeps it: allocated at the first use, grown if a later call
// needs more, freed with the handle.  Callers hold the mutex and have waited for `done`.
int64_t piece_rows(const clipgpu_index* ix) { return std::max<int64_t>(1, (64LL << 20) / (ix->E * 4)); }
float* scratch_bytes(clipgpu_index* ix, size_t need) {
  if (need > ix->scratch_bytes) {
    if (ix->scratch) HIP_CHECK(hipFree(ix->scratch));
    ix->scratch = nullptr;
    ix->scratch_bytes = 0;
    HIP_CHECK(hipMalloc((void**)&ix->scratch, need));
    ix->scratch_bytes = need;
  }
  return ix->scratch;
}
float* scratch_for(clipgpu_index* ix, int64_t rows) { return scratch_bytes(ix, (size_t)rows * ix->E * 4); }

}  // namespace

extern "C" {

int clipgpu_index_create(int device, int64_t E, int64_t capacity, clipgpu_index** out) {
  return clipgpu_index_create_ex(device, E, capacity, CLIPGPU_INDEX_F32, out);
}

int clipgpu_index_create_ex(int device, int64_t E, int64_t capacity, int dtype, clipgpu_index** out) {
  return guarded([&]() {
    if (!out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL out");
    *out = nullptr;
    if (dtype != CLIPGPU_INDEX_F32 && dtype != CLIPGPU_INDEX_F16 && dtype != CLIPGPU_INDEX_BF16)
      throw ClipErr(CLIPGPU_ERR_INVALID, "unknown index dtype");
    if (E <= 0 || E % 16) throw ClipErr(CLIPGPU_ERR_INVALID, "Shape error: embedding dim must be a multiple of 16");
    if (capacity <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "capacity must be positive");
    if (capacity >= (1LL << 31) || E > (1 << 20) || capacity > (1LL << 46) / (E * 4))
      throw ClipErr(CLIPGPU_ERR_INVALID, "Shape error: index too large (capacity < 2^31 rows)");
    if (device < 0) throw ClipErr(CLIPGPU_ERR_INVALID, "bad device");
    HIP_CHECK(hipSetDevice(device));
    clipgpu_index* ix = new clipgpu_index;
    ix->device = device;
    ix->E = E;
    ix->capacity = capacity;
    ix->dtype = dtype;
    ix->esz = topk_gal_bytes(dtype);
    ix->ws_blocks = (int)std::min<int64_t>(kMaxBlocks, 4 * ((capacity + 63) / 64));
    const size_t ws = align256((size_t)ix->ws_blocks * 64 * kTopkMax * 8);
    const size_t sq = align256((size_t)kQueryChunk * E * 4), si = align256((size_t)kQueryChunk * kTopkMax * 8);
    const size_t ss = align256((size_t)kQueryChunk * kTopkMax * 4);
    const size_t sl = align256((size_t)live_words(capacity) * 4), se = align256((size_t)topk_mask_words(capacity) * 4);
    const size_t sm = align256((size_t)ix->ws_blocks * 64 * 8), sn = align256((size_t)kQueryChunk * 2 * 4);
    hipError_t err = hipMalloc((void**)&ix->gallery, (size_t)capacity * E * ix->esz);
    if (err == hipSuccess) err = hipMalloc((void**)&ix->work, ws + sq + si + ss + sl + se + sm + ss + sn);
    if (err == hipSuccess) err = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&ix->done, hipEventDisableTiming);
    if (err != hipSuccess) {
      clipgpu_index_destroy(ix);
      HIP_CHECK(err);
    }
    ix->st_q = (float*)(ix->work + ws);
    ix->st_idx = (int64_t*)(ix->work + ws + sq);
    ix->st_score = (float*)(ix->work + ws + sq + si);
    ix->d_live = (uint32_t*)(ix->work + ws + sq + si + ss);
    ix->d_eff = (uint32_t*)(ix->work + ws + sq + si + ss + sl);
    ix->d_ms = ix->work + ws + sq + si + ss + sl + se;
    ix->st_prob = (float*)(ix->work + ws + sq + si + ss + sl + se + sm);
    ix->st_norm = (float*)(ix->work + ws + sq + si + ss + sl + se + sm + ss);
    *out = ix;
  });
}

void clipgpu_index_destroy(clipgpu_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  if (ix->done) {
    (void)hipEventSynchronize(ix->done);  // the last operation has left the buffers
    (void)hipEventDestroy(ix->done);
  }
  if (ix->stream) (void)hipStreamDestroy(ix->stream);
  if (ix->scratch) (void)hipFree(ix->scratch);
  if (ix->work) (void)hipFree(ix->work);
  if (ix->gallery) (void)hipFree(ix->gallery);
  delete ix;
}

int64_t clipgpu_index_size(const clipgpu_index* ix) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lk(const_cast<clipgpu_index*>(ix)->mu);
  return ix->size;
}

int clipgpu_index_clear(clipgpu_index* ix) {
  return guarded([&]() {
    if (!ix) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->size = 0;  // a later add overwrites the rows only after the last search (the `done` event)
    ix->h_live = std::vector<uint32_t>();  // every future row is live
    ix->n_dead = 0;
  });
}

int64_t clipgpu_index_live(const clipgpu_index* ix) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lk(const_cast<clipgpu_index*>(ix)->mu);
  return ix->size - ix->n_dead;
}

int clipgpu_index_get_live(clipgpu_index* ix, int64_t first, int64_t n, uint8_t* out) {
  return guarded([&]() {
    if (!ix || !out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (first < 0 || n <= 0 || n > ix->size || first > ix->size - n)
      throw ClipErr(CLIPGPU_ERR_INVALID, "rows out of range (first >= 0, n >= 1, first + n <= size)");
    for (int64_t i = 0; i < n; ++i) out[i] = is_live(ix, first + i) ? 1 : 0;
  });
}

int clipgpu_index_remove(clipgpu_index* ix, const int64_t* ids, int64_t n) {
  return guarded([&]() {
    check_ids(ix, ids, n);
    std::lock_guard<std::mutex> lk(ix->mu);
    check_ids_in_range(ix, ids, n);  // before any change and any device work
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    if (ix->h_live.empty()) {  // the first removal: every row, present and future, starts live
      ix->h_live.assign((size_t)live_words(ix->capacity), ~0u);
      HIP_CHECK(hipMemsetAsync(ix->d_live, 0xff, (size_t)live_words(ix->capacity) * 4, ix->stream));
      HIP_CHECK(hipStreamSynchronize(ix->stream));
    }
    bool changed = false;
    for (int64_t i = 0; i < n; ++i) {
      uint32_t& w = ix->h_live[ids[i] >> 5];
      const uint32_t bit = 1u << (ids[i] & 31);
      if (w & bit) {
        w &= ~bit;
        ++ix->n_dead;
        changed = true;
      }
    }
    if (changed) upload_live(ix);
    mark_last(ix, ix->stream);
  });
}

int clipgpu_index_set_rows(clipgpu_index* ix, const int64_t* ids, const float* rows, int64_t n) {
  return guarded([&]() {
    check_ids(ix, ids, n);
    if (!rows && n > 0) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    check_ids_in_range(ix, ids, n);
    {
      std::vector<int64_t> sorted(ids, ids + n);
      std::sort(sorted.begin(), sorted.end());
      if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        throw ClipErr(CLIPGPU_ERR_INVALID, "duplicate id");
    }
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    // pieces of f32 rows followed by their ids go through the device scratch; a scatter kernel writes
    // (and for a 16-bit index rounds, as add does) row ids[i]
    const int64_t piece = std::min(n, piece_rows(ix));
    const size_t row_bytes = (size_t)piece * ix->E * 4;  // a multiple of 64: the ids behind are aligned
    float* f32 = scratch_bytes(ix, row_bytes + (size_t)piece * 8);
    int64_t* d_ids = (int64_t*)((char*)f32 + row_bytes);
    for (int64_t r0 = 0; r0 < n; r0 += piece) {
      const int64_t m = std::min(piece, n - r0);
      HIP_CHECK(copy_h2d(f32, rows + r0 * ix->E, (size_t)m * ix->E * 4));
      HIP_CHECK(copy_h2d(d_ids, ids + r0, (size_t)m * 8));
      HIP_CHECK(launch_gal_scatter(ix->dtype, f32, d_ids, ix->gallery, m, (int)ix->E, ix->stream));
      HIP_CHECK(hipStreamSynchronize(ix->stream));
    }
    if (!ix->h_live.empty()) {  // the rows are live again
      bool changed = false;
      for (int64_t i = 0; i < n; ++i) {
        uint32_t& w = ix->h_live[ids[i] >> 5];
        const uint32_t bit = 1u << (ids[i] & 31);
        if (!(w & bit)) {
          w |= bit;
          --ix->n_dead;
          changed = true;
        }
      }
      if (changed) upload_live(ix);
    }
    mark_last(ix, ix->stream);
  });
}

int clipgpu_index_add_device(clipgpu_index* ix, const float* d_rows, int64_t n, void* stream) {
  return guarded([&]() {
    check_add(ix, d_rows, n);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (n > ix->capacity - ix->size) throw ClipErr(CLIPGPU_ERR_INVALID, "index full");
    HIP_CHECK(hipSetDevice(ix->device));
    hipStream_t s = (hipStream_t)stream;
    order_after_last(ix, s);
    char* dst = ix->gallery + ix->size * ix->E * ix->esz;
    if (ix->dtype == CLIPGPU_INDEX_F32)
      HIP_CHECK(hipMemcpyAsync(dst, d_rows, (size_t)n * ix->E * 4, hipMemcpyDeviceToDevice, s));
    else
      HIP_CHECK(launch_gal_round(ix->dtype, d_rows, dst, n * ix->E, s));
    mark_last(ix, s);
    ix->size += n;
  });
}

int clipgpu_index_add(clipgpu_index* ix, const float* rows, int64_t n) {
  return guarded([&]() {
    check_add(ix, rows, n);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (n > ix->capacity - ix->size) throw ClipErr(CLIPGPU_ERR_INVALID, "index full");
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    char* dst = ix->gallery + ix->size * ix->E * ix->esz;
    if (ix->dtype == CLIPGPU_INDEX_F32) {
      HIP_CHECK(copy_h2d(dst, rows, (size_t)n * ix->E * 4));
    } else {  // the f32 rows go to device scratch and are rounded there
      const int64_t piece = std::min(n, piece_rows(ix));
      float* f32 = scratch_for(ix, piece);
      for (int64_t r0 = 0; r0 < n; r0 += piece) {
        const int64_t m = std::min(piece, n - r0);
        HIP_CHECK(copy_h2d(f32, rows + r0 * ix->E, (size_t)m * ix->E * 4));
        HIP_CHECK(launch_gal_round(ix->dtype, f32, dst + r0 * ix->E * ix->esz, m * ix->E, ix->stream));
        HIP_CHECK(hipStreamSynchronize(ix->stream));
      }
    }
    ix->size += n;
  });
}

int clipgpu_index_dtype(const clipgpu_index* ix) { return ix ? ix->dtype : -1; }

int clipgpu_index_get_rows(clipgpu_index* ix, int64_t first, int64_t n, float* out_rows) {
  return guarded([&]() {
    if (!ix || !out_rows) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (first < 0 || n <= 0 || n > ix->size || first > ix->size - n)
      throw ClipErr(CLIPGPU_ERR_INVALID, "rows out of range (first >= 0, n >= 1, first + n <= size)");
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    const char* src = ix->gallery + first * ix->E * ix->esz;
    if (ix->dtype == CLIPGPU_INDEX_F32) {
      HIP_CHECK(copy_d2h(out_rows, src, (size_t)n * ix->E * 4));
      return;
    }
    const int64_t piece = std::min(n, piece_rows(ix));
    float* f32 = scratch_for(ix, piece);
    for (int64_t r0 = 0; r0 < n; r0 += piece) {
      const int64_t m = std::min(piece, n - r0);
      HIP_CHECK(launch_gal_widen(ix->dtype, src + r0 * ix->E * ix->esz, f32, m * ix->E, ix->stream));
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(out_rows + r0 * ix->E, f32, (size_t)m * ix->E * 4));
    }
  });
}

int clipgpu_index_search_filtered_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                         float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t* d_idx,
                                         float* d_score, void* stream) {
  return guarded([&]() {
    check_search(ix, d_queries, nq, k, d_idx, d_score);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // an empty gallery
    HIP_CHECK(hipSetDevice(ix->device));
    hipStream_t s = (hipStream_t)stream;
    order_after_last(ix, s);
    const uint32_t* mask = build_mask(ix, d_allow, s);
    search_on(ix, d_queries, nq, k, logit_scale, logit_bias, mask, d_idx, d_score, s);
  });
}

int clipgpu_index_search_filtered(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                                  float logit_bias, const uint32_t* allow, int64_t* out_idx, float* out_score) {
  return guarded([&]() {
    check_search(ix, queries, nq, k, out_idx, out_score);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    // the caller's words that hold rows [0, size) are staged where the filter is built, once for all chunks
    if (allow) HIP_CHECK(copy_h2d(ix->d_eff, allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, allow ? ix->d_eff : nullptr, ix->stream);
    for (int64_t q0 = 0; q0 < nq; q0 += kQueryChunk) {
      const int64_t rows = std::min(kQueryChunk, nq - q0);
      HIP_CHECK(copy_h2d(ix->st_q, queries + q0 * ix->E, (size_t)rows * ix->E * 4));
      search_on(ix, ix->st_q, rows, k, logit_scale, logit_bias, mask, ix->st_idx, ix->st_score, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(out_idx + q0 * k, ix->st_idx, (size_t)rows * k * 8));
      HIP_CHECK(copy_d2h(out_score + q0 * k, ix->st_score, (size_t)rows * k * 4));
    }
  });
}

int clipgpu_index_search_probs_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                      float logit_scale, float logit_bias, int activation, const uint32_t* d_allow,
                                      int64_t* d_idx, float* d_score, float* d_prob, float* d_norm, void* stream) {
  return guarded([&]() {
    const int probs = probs_kind(activation);
    check_search(ix, d_queries, nq, k, d_idx, d_score);
    if (!d_prob) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
    HIP_CHECK(hipSetDevice(ix->device));
    hipStream_t s = (hipStream_t)stream;
    order_after_last(ix, s);
    const uint32_t* mask = build_mask(ix, d_allow, s);
    search_on(ix, d_queries, nq, k, logit_scale, logit_bias, mask, d_idx, d_score, s, probs, d_prob,
              probs == TOPK_PROBS_SOFTMAX ? d_norm : nullptr);
  });
}

int clipgpu_index_search_probs(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                               float logit_bias, int activation, const uint32_t* allow, int64_t* out_idx,
                               float* out_score, float* out_prob, float* out_norm) {
  return guarded([&]() {
    const int probs = probs_kind(activation);
    check_search(ix, queries, nq, k, out_idx, out_score);
    if (!out_prob) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    if (allow) HIP_CHECK(copy_h2d(ix->d_eff, allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, allow ? ix->d_eff : nullptr, ix->stream);
    const bool norm = out_norm && probs == TOPK_PROBS_SOFTMAX;
    for (int64_t q0 = 0; q0 < nq; q0 += kQueryChunk) {
      const int64_t rows = std::min(kQueryChunk, nq - q0);
      HIP_CHECK(copy_h2d(ix->st_q, queries + q0 * ix->E, (size_t)rows * ix->E * 4));
      search_on(ix, ix->st_q, rows, k, logit_scale, logit_bias, mask, ix->st_idx, ix->st_score, ix->stream, probs,
                ix->st_prob, norm ? ix->st_norm : nullptr);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(out_idx + q0 * k, ix->st_idx, (size_t)rows * k * 8));
      HIP_CHECK(copy_d2h(out_score + q0 * k, ix->st_score, (size_t)rows * k * 4));
      HIP_CHECK(copy_d2h(out_prob + q0 * k, ix->st_prob, (size_t)rows * k * 4));
      if (norm) HIP_CHECK(copy_d2h(out_norm + q0 * 2, ix->st_norm, (size_t)rows * 2 * 4));
    }
  });
}

int clipgpu_index_search_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k, float logit_scale,
                                float logit_bias, int64_t* d_idx, float* d_score, void* stream) {
  return clipgpu_index_search_filtered_device(ix, d_queries, nq, k, logit_scale, logit_bias, nullptr, d_idx, d_score,
                                              stream);
}

int clipgpu_index_search(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                         float logit_bias, int64_t* out_idx, float* out_score) {
  return clipgpu_index_search_filtered(ix, queries, nq, k, logit_scale, logit_bias, nullptr, out_idx, out_score);
}

}  // extern "C"
