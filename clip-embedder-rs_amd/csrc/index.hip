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
// other search runs the unmasked kernels.
//
// Probabilities (clipgpu_index_search_probs).  The same search with one more output, the softmax over the
// searched rows or the sigmoid of the k results.  The softmax needs one (max, sum) pair per (query row,
// span); they live in the work area too (64 pairs per phase-1 block the workspace holds), as do the host
// form's staged probabilities and (max, sum) rows.
// Every search entry point fills a SearchReq and a SearchOut for one of two workers, search_device or
// search_host.  A 16-bit gallery's rows are converted by kernels/gallery.hip on their way in and out.
//
// Range search and self-join (clipgpu_index_range_search[_device], clipgpu_index_self_join; kernels/range.hip).
// The same chunks of 256 query rows, route and span cut as a search, but every chunk appends its hits to one
// bounded record buffer behind one 64-bit counter.  The device form writes the caller's buffers; the host forms
// use a record buffer of the handle's (allocated at the first such call, grown on demand), sort the records on
// the host and refuse an overflow with the exact total.
//
// Assignment and k-means (clipgpu_index_assign[_device], clipgpu_index_kmeans; kernels/cluster.hip).  One launch
// assigns every slot under the search's mask; there is no span cut and no chunking, a block owns 64 gallery
// rows.  k-means alternates that launch with an integer-sum update and reads one counter back per iteration;
// its labels, scores, centroids and sums live in buffers of the handle's, lazy like the record buffer.
//
// Labelling (clipgpu_index_classify[_device]; kernels/classify.hip).  The assignment's launch with the k best labels
// of every slot, k <= 16, and their softmax or sigmoid probabilities; the host form's labels share the assignment's
// centroid buffer and its outputs have a lazy buffer of their own.
//
// Inverted lists and the probed search (clipgpu_index_partition, clipgpu_index_search_probed[_device];
// kernels/lists.hip, kernels/probe.hip).  partition assigns the live rows to the given centroids and sorts their
// ids by label into CSR lists (device) whose offsets it also keeps on the host; add, add_device, set_rows and
// clear mark the partition stale, remove does not (the live bit rejects the row at search time).  A probed
// search is, per chunk of queries: a coarse launch_topk over the handle's centroid copy, the probe kernel over
// (query, probed list, part of the list) into the search workspace, and the search's merge.  The parts per list
// and the rows per chunk come from the host's offsets and the workspace's size, so nothing synchronises.
//
// Int8 codes and the coded search (clipgpu_index_enable_codes, clipgpu_index_search_coded[_device];
// kernels/codes.hip).  Once enabled, the codes are a second device array beside the gallery: add, add_device and
// set_rows code the rows they write, on the same stream, after the gallery write.  A coded search is, per chunk
// of queries: the queries' codes, the coarse scan of the gallery's codes and the search's merge with k = refine
// (the candidates), then the probe kernel over each query's candidates as a list of its own and the merge again.
// An index whose codes were never enabled runs none of this.
//
// Deep search (clipgpu_index_search_deep[_device]; kernels/deep.hip): the search for k up to 4096.  The same
// chunks, route and span cut as a search; per chunk launch_deep enqueues its fixed sequence of launches into a
// work area of the handle's (the chunk's histograms, state and candidate records, and the host form's staged
// results), allocated at the first deep search and kept until the handle is destroyed.
//
// Compound queries (clipgpu_index_search_compound[_device]; kernels/compound.hip): a query is a group of 1 .. 16
// terms, scored by the smallest or the largest of its term logits.  The same chunks of 256 queries; per chunk a
// gather pads the groups to the chunk's slot width into a buffer of the handle's (lazy, as the deep search's),
// the compound phase 1 fills the search workspace and the search's merge writes the result.
//
// Group labels and the grouped search (clipgpu_index_set_groups, clipgpu_index_groups,
// clipgpu_index_search_grouped[_device]; kernels/grouped.hip).  One uint32 label per slot of the capacity and,
// behind them, the host form's staged groups: one buffer, allocated and filled with "ungrouped" at the first
// set_groups or grouped search and kept until the handle is destroyed; an index that never calls either has none.
// add leaves new rows ungrouped, set_rows and remove keep a slot's label, clear resets every label.  A grouped
// search is the same chunks of 256 queries, the compound search's span cut at width 1, one launch_grouped each.
//
// Diversified search (clipgpu_index_search_diverse[_device]; kernels/diverse.hip): per chunk of 256 queries a
// search for the pool of P candidates into an area of the handle's (or the caller's pool buffers), then
// launch_diverse, which fills the chunk's Gram matrices [rows][P][P] behind the pool and selects.  The area is
// lazy, grown when a call brings a larger P, kept until the handle is destroyed.
//
// Neighbours of stored rows and the k-NN graph (clipgpu_index_neighbors[_device]; kernels/knn.hip): the query rows
// are gallery rows, named by id or every slot.  One span cut per call (knn_plan), then as many launches of
// launch_knn as the search workspace asks for; the device form writes the caller's buffers, the host form stages
// pieces of 8192 rows in an area of the handle's, lazy and kept like the others.
//
// Duplicate groups (clipgpu_index_components[_device]; kernels/components.hip): the connected components of the
// self-join's threshold graph.  One launch_components per call -- init, join-and-hook, flatten -- on one stream
// under the search's mask, with no chunk loop and nothing read back in between.  The union-find's parent array
// (int32 per slot of the capacity) and, behind it, the host form's staged labels and the counter are one buffer of
// the handle's, allocated at the first call and kept until the handle is destroyed.  to_groups has the flatten
// write the group labels as well (allocated as set_groups allocates them).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/clipgpu.h"
#include "bounce.hpp"
#include "hip_check.hpp"
#include "host/api_util.hpp"
#include "kernels/kernels.hpp"
#include "kernels/topk_key.hpp"

using namespace clipgpu;

namespace {

constexpr int64_t kQueryChunk = 256;  // queries per launch: 4 query tiles
constexpr int kMaxBlocks = 1024;      // phase-1 blocks per launch the workspace is sized for (4 per CU)
inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

// Test hooks of the probed search (clipgpu_test_probe_parts, clipgpu_test_probe_chunk); 0 = the default.
std::atomic<int> g_probe_parts{0};
std::atomic<int> g_probe_chunk{0};
// Test hook of the coded search (clipgpu_test_codes_stage): 0 = both stages, 1 = the coarse stage only, 2 = the
// re-rank only, on the candidates the last coarse stage left.
std::atomic<int> g_codes_stage{0};

}  // namespace

struct clipgpu_index {
  std::mutex mu;
  int device = 0;
  int64_t E = 0, capacity = 0, size = 0;
  int dtype = CLIPGPU_INDEX_F32;  // the gallery's element type
  int64_t esz = 4;                // its bytes
  char* gallery = nullptr;        // [capacity][E] of esz bytes
  int ws_blocks = 0;         // phase-1 blocks the workspace holds: min(kMaxBlocks, 4 * 64-row tiles of capacity)
  char* work = nullptr;      // one allocation; its regions, in the order carve_work places them:
  void* d_ws = nullptr;          // the search workspace: ws_blocks * 64 rows of kTopkMax entries
  float* st_q = nullptr;         // the host form's staged query chunk [kQueryChunk][E],
  int64_t* st_idx = nullptr;     // its indices [kQueryChunk][kTopkMax]
  float* st_score = nullptr;     // and scores
  uint32_t* d_live = nullptr;    // the mirror of h_live; bits at and past `size` are ones; read only while n_dead > 0
  uint32_t* d_eff = nullptr;     // the filter of the search in flight: live & allow, whole 64-row tiles
  void* d_ms = nullptr;          // the softmax search in flight: one (max, sum) per (query row, span), 64 * ws_blocks
  float* st_prob = nullptr;      // the host form's staged probabilities [kQueryChunk][kTopkMax]
  float* st_norm = nullptr;      // and (max, sum) rows [kQueryChunk][2]
  std::vector<uint32_t> h_live;  // bit i: row i is live; ceil(capacity / 32) words, empty = every row live
  int64_t n_dead = 0;            // cleared bits of h_live below `size`
  float* scratch = nullptr;      // 16-bit index: f32 rows on their way in (add) or out (get_rows); lazy
  size_t scratch_bytes = 0;
  char* res = nullptr;           // range search / self-join, host forms: the counter and res_records records; lazy
  int64_t res_records = 0;
  // assign (host form) and kmeans; lazy, grown on demand, carved by cluster_buffers:
  char* cl_rows = nullptr;       // a ClusterStat, two generations of int32 labels and the scores, cl_rows_n rows each
  int64_t cl_rows_n = 0;
  char* cl_cen = nullptr;        // the centroids f32 [cl_cen_n][E]
  int64_t cl_cen_n = 0;
  char* cl_sum = nullptr;        // kmeans: the sums int64 [cl_sum_n][E]
  int64_t cl_sum_n = 0;
  int64_t km_C = 0;              // the last update's centroid count (0 = none yet) and shift, for
  int km_shift = 0;              // clipgpu_test_index_kmeans_sums
  // the partition (clipgpu_index_partition); lazy, grown on demand, freed with the handle:
  char* pt_ids = nullptr;        // the lists' row ids int32 [pt_ids_n]
  int64_t pt_ids_n = 0;
  char* pt_off = nullptr;        // their offsets int32 [pt_off_n + 1]
  int64_t pt_off_n = 0;
  char* pt_cen = nullptr;        // the partition's own copy of the centroids f32 [pt_cen_n][E]
  int64_t pt_cen_n = 0;
  char* pt_coarse = nullptr;     // the coarse step of a probed search: indices int64 and scores f32
                                 // [kQueryChunk][kTopkMax], and the host form's staged probes (int64, as many)
  int64_t pt_C = 0;              // the lists of the partition in force; 0 = none
  bool pt_stale = false;         // rows were added, replaced or cleared since
  std::vector<int32_t> pt_h_off; // the offsets on the host [pt_C + 1]
  int64_t pt_longest = 0;        // the longest list
  // the int8 codes (clipgpu_index_enable_codes); allocated there, freed by drop_codes or with the handle:
  int8_t* cd_codes = nullptr;    // [capacity][cd_Ep], cd_Ep = E rounded up to 64; NULL = no codes
  float* cd_scale = nullptr;     // [capacity]
  char* cd_work = nullptr;       // a coded search in flight: the regions carve_codes places
  int64_t cd_Ep = 0;
  char* dp_work = nullptr;       // the deep search: what deep_buffers carves; lazy, kept until the handle is destroyed
  char* cp_work = nullptr;       // compound queries: what compound_buffers places; lazy, kept likewise
  int64_t cp_work_n = 0;
  char* gp_labels = nullptr;     // group labels uint32 [capacity], then the host form's staged groups int64
                                 // [kQueryChunk][kTopkMax]; lazy, kept likewise; NULL = every row ungrouped
  char* dv_work = nullptr;       // the diversified search: what diverse_buffers places, for pools up to dv_work_n;
  int64_t dv_work_n = 0;         // lazy, grown on demand, kept likewise
  char* kn_work = nullptr;       // neighbours, host form: a piece's ids, indices and scores (KnnWork), kn_work_n rows;
  int64_t kn_work_n = 0;         // lazy, kept likewise
  char* cc_work = nullptr;       // duplicate groups: parent int32 [capacity], the host form's labels int32 [capacity]
                                 // and the counter (CcBuf); lazy, kept likewise
  char* cf_work = nullptr;       // classify, host form: labels int32, scores, probabilities and (max, sum) rows f32,
  int64_t cf_work_n = 0;         // cf_work_n entries each (classify_buffers); lazy, grown on demand, kept likewise
  hipStream_t stream = nullptr;  // the host-buffer forms' stream
  hipEvent_t done = nullptr;     // recorded after every device-side operation
};

namespace {

void order_after_last(clipgpu_index* ix, hipStream_t s) { HIP_CHECK(hipStreamWaitEvent(s, ix->done, 0)); }
void mark_last(clipgpu_index* ix, hipStream_t s) { HIP_CHECK(hipEventRecord(ix->done, s)); }

int64_t live_words(int64_t rows) { return (rows + 31) / 32; }
bool is_live(const clipgpu_index* ix, int64_t i) { return ix->h_live.empty() || ((ix->h_live[i >> 5] >> (i & 31)) & 1u); }

// The next region of the work area: `bytes` at base + off (base NULL: sizes only); off stays a multiple of 256.
template <typename T>
T* carve(char* base, size_t& off, size_t bytes) {
  T* p = base ? (T*)(base + off) : nullptr;
  off += align256(bytes);
  return p;
}

// The work area's layout, once: places the regions at `base` (NULL: nowhere yet) and returns the area's bytes.
// hipMalloc aligns the base to 256 bytes at least, so every region is; d_eff and d_ms need 8.
size_t carve_work(clipgpu_index* ix, char* base) {
  size_t off = 0, chunk = (size_t)kQueryChunk;
  ix->d_ws = carve<char>(base, off, (size_t)ix->ws_blocks * 64 * kTopkMax * 8);
  ix->st_q = carve<float>(base, off, chunk * ix->E * 4);
  ix->st_idx = carve<int64_t>(base, off, chunk * kTopkMax * 8);
  ix->st_score = carve<float>(base, off, chunk * kTopkMax * 4);
  ix->d_live = carve<uint32_t>(base, off, (size_t)live_words(ix->capacity) * 4);
  ix->d_eff = carve<uint32_t>(base, off, (size_t)topk_mask_words(ix->capacity) * 4);
  ix->d_ms = carve<char>(base, off, (size_t)ix->ws_blocks * 64 * 8);
  ix->st_prob = carve<float>(base, off, chunk * kTopkMax * 4);
  ix->st_norm = carve<float>(base, off, chunk * 2 * 4);
  return off;
}

void check_add(const clipgpu_index* ix, const float* rows, int64_t n) {
  if (!ix || !rows) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (n <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
}
char* append_at(const clipgpu_index* ix, int64_t n) {  // where n more rows go; refused if they do not fit
  if (n > ix->capacity - ix->size) throw ClipErr(CLIPGPU_ERR_INVALID, "index full");
  return ix->gallery + ix->size * ix->E * ix->esz;
}
void check_row_range(const clipgpu_index* ix, int64_t first, int64_t n) {
  if (first < 0 || n <= 0 || n > ix->size || first > ix->size - n)
    throw ClipErr(CLIPGPU_ERR_INVALID, "rows out of range (first >= 0, n >= 1, first + n <= size)");
}

// One search call: what is asked, and where the results go.  Device pointers for search_device and search_on,
// host pointers for search_host.  q [nq][E]; probs: TOPK_PROBS_*; allow: the caller's words or NULL.
struct SearchReq { const float* q; int64_t nq, k; float scale, bias; int probs; const uint32_t* allow; };
// idx, score, prob: [nq][k], prob for a probability search only; norm: [nq][2] or NULL, written by softmax only.
struct SearchOut { int64_t* idx; float* score; float* prob; float* norm; };

// The activation of a probability search as the kernels name it, or kBadActivation.
constexpr int kBadActivation = -1;
int probs_kind(int activation) {
  if (activation == CLIPGPU_SIM_SOFTMAX) return TOPK_PROBS_SOFTMAX;
  return activation == CLIPGPU_SIM_SIGMOID ? TOPK_PROBS_SIGMOID : kBadActivation;
}

// The refusals that need no lock (the activation before the handle is looked at, NULL arguments, the batch,
// k, then the probabilities' buffer); then the lock, the empty gallery, and the handle's device.
std::unique_lock<std::mutex> enter_search(clipgpu_index* ix, const SearchReq& r, const SearchOut& o) {
  if (r.probs == kBadActivation)
    throw ClipErr(CLIPGPU_ERR_INVALID, "activation must be CLIPGPU_SIM_SOFTMAX or CLIPGPU_SIM_SIGMOID "
                                       "(logits: clipgpu_index_search_filtered)");
  if (!ix || !r.q || !o.idx || !o.score) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (r.nq <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (r.k < 1 || r.k > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k must be in 1.." + std::to_string(CLIPGPU_TOPK_MAX) +
                                           " (clipgpu_similarity gives the whole matrix)");
  if (r.probs != TOPK_PROBS_NONE && !o.prob) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // an empty gallery
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

// The filter of one search call, written on `s` (which the caller has ordered after the handle's last
// operation): NULL if nothing filters (no allow bitmap, no removed row), else d_eff = live & allow.
// d_allow: device words (d_eff itself for the host form, which stages its bitmap there) or NULL.
const uint32_t* build_mask(clipgpu_index* ix, const uint32_t* d_allow, hipStream_t s) {
  if (!d_allow && ix->n_dead == 0) return nullptr;
  HIP_CHECK(launch_topk_mask(ix->n_dead ? ix->d_live : nullptr, d_allow, ix->d_eff, ix->size, s));
  return ix->d_eff;
}

// Searches the device rows r.q in chunks of kQueryChunk rows on `s`, all under one mask, into the device buffers
// of `o`.  The span cut is the same with and without probabilities: a launch of B phase-1 blocks writes at most
// 64 B pairs (wide: 64 rows per block; few-query: 16 rows, at most 4 * ws_blocks spans), which the pair area holds.
void search_on(clipgpu_index* ix, const SearchReq& r, const uint32_t* mask, const SearchOut& o, hipStream_t s) {
  for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
    const int rows = (int)std::min(kQueryChunk, r.nq - q0);
    const TopkPlan p = topk_plan(ix->size, rows, ix->ws_blocks);  // the route too: few rows, few-query kernel
    HIP_CHECK(launch_topk({r.q + q0 * ix->E, rows, ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, r.scale, r.bias,
                           (int)r.k, p, ix->d_ws, mask, o.idx + q0 * r.k, o.score + q0 * r.k, r.probs, ix->d_ms,
                           64L * ix->ws_blocks, o.prob ? o.prob + q0 * r.k : nullptr,
                           o.norm ? o.norm + q0 * 2 : nullptr, s}));
  }
  mark_last(ix, s);
}

// The device form: on the caller's stream, ordered after the handle's last operation; r.allow is device words.
int search_device(clipgpu_index* ix, const SearchReq& r, const SearchOut& o, hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_search(ix, r, o);
    order_after_last(ix, s);
    search_on(ix, r, build_mask(ix, r.allow, s), o, s);
  });
}

// The host form: a chunk of queries is staged, searched on the handle's stream and copied back.
int search_host(clipgpu_index* ix, const SearchReq& r, const SearchOut& o) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_search(ix, r, o);
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    // the caller's words that hold rows [0, size) are staged where the filter is built, once for all chunks
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    const bool norm = o.norm && r.probs == TOPK_PROBS_SOFTMAX;  // sigmoid writes none: o.norm stays as it is
    const SearchOut st = {ix->st_idx, ix->st_score, o.prob ? ix->st_prob : nullptr, norm ? ix->st_norm : nullptr};
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
      const SearchReq c = {ix->st_q, std::min(kQueryChunk, r.nq - q0), r.k, r.scale, r.bias, r.probs, nullptr};
      HIP_CHECK(copy_h2d(ix->st_q, r.q + q0 * ix->E, (size_t)c.nq * ix->E * 4));
      search_on(ix, c, mask, st, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(o.idx + q0 * r.k, st.idx, (size_t)c.nq * r.k * 8));
      HIP_CHECK(copy_d2h(o.score + q0 * r.k, st.score, (size_t)c.nq * r.k * 4));
      if (st.prob) HIP_CHECK(copy_d2h(o.prob + q0 * r.k, st.prob, (size_t)c.nq * r.k * 4));
      if (st.norm) HIP_CHECK(copy_d2h(o.norm + q0 * 2, st.norm, (size_t)c.nq * 2 * 4));
    }
  });
}

// The live words that hold rows [0, size) to the device mirror (synchronous).  Callers hold the mutex
// and have waited for `done`.
void upload_live(clipgpu_index* ix) {
  HIP_CHECK(copy_h2d(ix->d_live, ix->h_live.data(), (size_t)live_words(ix->size) * 4));
}

// Sets (live) or clears the bits of ids[0 .. n) in h_live (which exists), keeps n_dead; true if a bit changed.
bool mark_rows(clipgpu_index* ix, const int64_t* ids, int64_t n, bool live) {
  bool changed = false;
  for (int64_t i = 0; i < n; ++i) {
    uint32_t& w = ix->h_live[ids[i] >> 5];
    const uint32_t bit = 1u << (ids[i] & 31);
    if (((w & bit) != 0) != live) {
      w ^= bit;
      ix->n_dead += live ? -1 : 1;
      changed = true;
    }
  }
  return changed;
}

void check_ids(const clipgpu_index* ix, const int64_t* ids, int64_t n) {
  if (!ix || (!ids && n > 0)) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (n < 0) throw ClipErr(CLIPGPU_ERR_INVALID, "negative count");
}
void check_ids_in_range(const clipgpu_index* ix, const int64_t* ids, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= ix->size) throw ClipErr(CLIPGPU_ERR_INVALID, "id out of range (0 <= id < size)");
}

// Device scratch for host f32 rows on their way into or out of the gallery (add and get_rows of a 16-bit index,
// set_rows of any): allocated at the first use, grown if a later call needs more, freed with the handle.
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

// n rows through the scratch in pieces of at most 64 MiB of f32 (one row if a row is larger): f(r0, m, f32,
// behind) for rows [r0, r0 + m), with room for them at f32 and `extra` bytes per row behind (64-byte aligned).
// Callers hold the mutex and have waited for `done`; f leaves nothing in flight that uses the scratch.
template <typename F>
void for_each_piece(clipgpu_index* ix, int64_t n, size_t extra, F f) {
  const int64_t piece = std::min(n, std::max<int64_t>(1, (64LL << 20) / (ix->E * 4)));
  const size_t row_bytes = (size_t)piece * ix->E * 4;
  float* f32 = scratch_bytes(ix, row_bytes + (size_t)piece * extra);
  for (int64_t r0 = 0; r0 < n; r0 += piece) f(r0, std::min(piece, n - r0), f32, (char*)f32 + row_bytes);
}

// ---- range search and self-join (kernels/range.hip) ------------------------------------------------------
// One call: the threshold, the score's scale and bias, and the record capacity the kernels may write up to.
struct RangeReq { float thr, scale, bias; int64_t cap; };
// Where the records go, on the device: three arrays of `cap` entries and the 64-bit counter of all hits.
struct RangeBuf { int32_t* query; int32_t* row; float* score; unsigned long long* total; };

// The refusals that need no lock and no device, in the order the header lists them; then as enter_search.
// `what` names the capacity argument of the entry point.
std::unique_lock<std::mutex> enter_range(clipgpu_index* ix, bool null_arg, int64_t nq, const RangeReq& r,
                                         const char* what) {
  if (!ix || null_arg) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (nq <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (nq > INT32_MAX) throw ClipErr(CLIPGPU_ERR_INVALID, "too many queries (nq <= 2^31 - 1: a record holds an int32)");
  if (r.thr != r.thr) throw ClipErr(CLIPGPU_ERR_INVALID, "threshold must not be NaN");
  if (r.cap < 1 || r.cap > kRangeMaxRecords)
    throw ClipErr(CLIPGPU_ERR_INVALID, std::string(what) + " must be in 1.." + std::to_string(kRangeMaxRecords) +
                                           " (2^28), got " + std::to_string(r.cap));
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // an empty gallery
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

// One launch: `rows` query rows at q (device f32) whose records carry query indices q_off .. q_off + rows.
// join: they are the gallery rows q_off .. themselves, and the spans start at q_off & ~63.
void range_chunk(clipgpu_index* ix, const float* q, int rows, int64_t q_off, bool join, const RangeReq& r,
                 const uint32_t* mask, const RangeBuf& o, hipStream_t s) {
  const unsigned col0 = join ? (unsigned)(q_off & ~63LL) : 0u;
  const TopkPlan p = topk_plan(ix->size - col0, rows, ix->ws_blocks);  // the search's route and span cut
  HIP_CHECK(launch_range({q, rows, ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, r.scale, r.bias, r.thr, p, col0,
                          mask, (int)q_off, join, (long)r.cap, o.query, o.row, o.score, o.total, s}));
}

// The host forms' device records: allocated at the first use, grown when a call asks for more, freed with the
// handle.  A failed allocation is CLIPGPU_ERR_DEVICE and leaves the handle without the buffer, usable.
// Callers hold the mutex and have waited for `done`.
RangeBuf result_buffer(clipgpu_index* ix, int64_t records) {
  if (records > ix->res_records) {
    if (ix->res) HIP_CHECK(hipFree(ix->res));
    ix->res = nullptr;
    ix->res_records = 0;
    HIP_CHECK(hipMalloc((void**)&ix->res, 256 + 3 * align256((size_t)records * 4)));
    ix->res_records = records;
  }
  size_t off = 0;
  RangeBuf b;
  b.total = carve<unsigned long long>(ix->res, off, 8);
  b.query = carve<int32_t>(ix->res, off, (size_t)ix->res_records * 4);
  b.row = carve<int32_t>(ix->res, off, (size_t)ix->res_records * 4);
  b.score = carve<float>(ix->res, off, (size_t)ix->res_records * 4);
  return b;
}

struct RangeRec { int32_t query; uint32_t row, bits; };

// After the launches of a host form, on the handle's stream: waits, writes *out_total, refuses an overflow
// (`what` names the capacity argument) and returns the records sorted by (query, then less(a, b)).
template <typename Less>
std::vector<RangeRec> fetch_records(clipgpu_index* ix, const RangeBuf& b, int64_t cap, const char* what,
                                    int64_t* out_total, Less less) {
  HIP_CHECK(hipStreamSynchronize(ix->stream));
  unsigned long long total = 0;
  HIP_CHECK(copy_d2h(&total, b.total, 8));
  *out_total = (int64_t)total;
  if (total > (unsigned long long)cap)
    throw ClipErr(CLIPGPU_ERR_INVALID, "result overflow: " + std::to_string(total) + " results, " + what + " is " +
                                           std::to_string(cap) + " (retry with " + what + " >= " +
                                           std::to_string(total) + ")");
  const size_t n = (size_t)total;
  std::vector<int32_t> hq(n), hr(n);
  std::vector<float> hs(n);
  if (n) {
    HIP_CHECK(copy_d2h(hq.data(), b.query, n * 4));
    HIP_CHECK(copy_d2h(hr.data(), b.row, n * 4));
    HIP_CHECK(copy_d2h(hs.data(), b.score, n * 4));
  }
  std::vector<RangeRec> rec(n);
  for (size_t i = 0; i < n; ++i) {
    uint32_t bits;
    memcpy(&bits, &hs[i], 4);
    rec[i] = {hq[i], (uint32_t)hr[i], bits};
  }
  std::sort(rec.begin(), rec.end(), [&](const RangeRec& a, const RangeRec& c) {
    return a.query != c.query ? a.query < c.query : less(a, c);
  });
  return rec;
}

// ---- assignment and k-means (kernels/cluster.hip) --------------------------------------------------------
// A device buffer of the handle's for `need` entries of `bytes` in all: allocated at the first use, grown when
// a call needs more, freed with the handle.  A failed allocation is CLIPGPU_ERR_DEVICE and leaves the handle
// without the buffer, usable.  Callers hold the mutex and have waited for `done`.
void grow(char*& p, int64_t& have, int64_t need, size_t bytes) {
  if (need <= have) return;
  if (p) HIP_CHECK(hipFree(p));
  p = nullptr;
  have = 0;
  HIP_CHECK(hipMalloc((void**)&p, bytes));
  have = need;
}

struct ClusterBuf { ClusterStat* stat; int32_t* label[2]; float* score; float* cen; int64_t* sum; };

// The buffers of a host assign (sums = false) or a kmeans over the present rows and C centroids.
ClusterBuf cluster_buffers(clipgpu_index* ix, int64_t C, bool sums) {
  grow(ix->cl_rows, ix->cl_rows_n, ix->size, 256 + 3 * align256((size_t)ix->size * 4));
  grow(ix->cl_cen, ix->cl_cen_n, C, (size_t)C * ix->E * 4);
  if (sums && C > ix->cl_sum_n) {
    ix->km_C = 0;  // the sums of the last update go with the buffer
    grow(ix->cl_sum, ix->cl_sum_n, C, (size_t)C * ix->E * 8);
  }
  size_t off = 0;
  ClusterBuf b;
  b.stat = carve<ClusterStat>(ix->cl_rows, off, sizeof(ClusterStat));
  for (int g = 0; g < 2; ++g) b.label[g] = carve<int32_t>(ix->cl_rows, off, (size_t)ix->cl_rows_n * 4);
  b.score = carve<float>(ix->cl_rows, off, (size_t)ix->cl_rows_n * 4);
  b.cen = (float*)ix->cl_cen;
  b.sum = (int64_t*)ix->cl_sum;
  return b;
}

// The refusals that need no lock and no device; then as enter_search.
std::unique_lock<std::mutex> enter_cluster(clipgpu_index* ix, bool null_arg, int64_t C) {
  if (!ix || null_arg) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (C < 1 || C > kClusterMaxCentroids)
    throw ClipErr(CLIPGPU_ERR_INVALID, "the number of centroids must be in 1.." + std::to_string(kClusterMaxCentroids) +
                                           ", got " + std::to_string(C));
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // an empty gallery
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

void assign_on(clipgpu_index* ix, const float* d_cen, int64_t C, float scale, float bias, const uint32_t* mask,
               int32_t* d_label, float* d_score, hipStream_t s) {
  HIP_CHECK(launch_assign({ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, d_cen, (int)C, scale, bias, mask, d_label,
                           d_score, s}));
}

// The labels (widened to int64) and scores of every slot, after the handle's stream has run.
void fetch_assignment(clipgpu_index* ix, const int32_t* d_label, const float* d_score, int64_t* out_label,
                      float* out_score) {
  std::vector<int32_t> l((size_t)ix->size);
  HIP_CHECK(copy_d2h(l.data(), d_label, l.size() * 4));
  HIP_CHECK(copy_d2h(out_score, d_score, l.size() * 4));
  for (size_t i = 0; i < l.size(); ++i) out_label[i] = l[i];
}

// ---- labelling every stored row (kernels/classify.hip) ----------------------------------------------------
static_assert(kClassifyMaxK == CLIPGPU_CLASSIFY_K_MAX, "the header's limit is the kernel's");
struct ClassifyReq { const float* labels; int64_t C, k; float scale, bias; int probs; const uint32_t* allow; };
// Device pointers: the caller's for the device form, the regions of cf_work for the host form.
struct ClassifyBuf { int32_t* label; float* score; float* prob; float* norm; };

// The refusals that need no lock and no device (the activation, NULL arguments, C, then k); then as enter_cluster.
std::unique_lock<std::mutex> enter_classify(clipgpu_index* ix, const ClassifyReq& r, bool null_out) {
  if (r.probs == kBadActivation)
    throw ClipErr(CLIPGPU_ERR_INVALID, "activation must be CLIPGPU_SIM_SOFTMAX or CLIPGPU_SIM_SIGMOID");
  if (!ix || !r.labels || null_out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (r.C < 1 || r.C > kClusterMaxCentroids)
    throw ClipErr(CLIPGPU_ERR_INVALID, "the number of labels must be in 1.." + std::to_string(kClusterMaxCentroids) +
                                           ", got " + std::to_string(r.C));
  if (r.k < 1 || r.k > kClassifyMaxK)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k must be in 1.." + std::to_string(kClassifyMaxK) + ", got " +
                                           std::to_string(r.k));
  return enter_cluster(ix, false, r.C);
}

void classify_on(clipgpu_index* ix, const ClassifyReq& r, const float* d_labels, const uint32_t* mask,
                 const ClassifyBuf& o, hipStream_t s) {
  HIP_CHECK(launch_classify({ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, d_labels, (int)r.C, (int)r.k, r.scale,
                             r.bias, r.probs, mask, o.label, o.score, o.prob, o.norm, s}));
}

// The host form's device outputs for the present rows at depth k.
ClassifyBuf classify_buffers(clipgpu_index* ix, int64_t k) {
  const int64_t n = ix->size * std::max<int64_t>(k, 2);  // four regions of n entries: the last holds [size][2]
  grow(ix->cf_work, ix->cf_work_n, n, 4 * align256((size_t)n * 4));
  size_t off = 0;
  ClassifyBuf b;
  b.label = carve<int32_t>(ix->cf_work, off, (size_t)ix->cf_work_n * 4);
  b.score = carve<float>(ix->cf_work, off, (size_t)ix->cf_work_n * 4);
  b.prob = carve<float>(ix->cf_work, off, (size_t)ix->cf_work_n * 4);
  b.norm = carve<float>(ix->cf_work, off, (size_t)ix->cf_work_n * 4);
  return b;
}


// ---- the partition and the probed search (kernels/lists.hip, kernels/probe.hip) ---------------------------
// The regions of pt_coarse.
constexpr size_t kCoarseEntries = (size_t)kQueryChunk * kTopkMax;
int64_t* coarse_idx(clipgpu_index* ix) { return (int64_t*)ix->pt_coarse; }
float* coarse_score(clipgpu_index* ix) { return (float*)(ix->pt_coarse + kCoarseEntries * 8); }
int64_t* coarse_probes(clipgpu_index* ix) { return (int64_t*)(ix->pt_coarse + kCoarseEntries * 12); }

void drop_partition(clipgpu_index* ix) {
  ix->pt_C = 0;
  ix->pt_stale = false;
  ix->pt_h_off = std::vector<int32_t>();
  ix->pt_longest = 0;
}

// One probed search call.  q, allow and the outputs: device pointers for probed_on and probed_device, host
// pointers for probed_host.  probes: [nq][nprobe] or NULL.
struct ProbedReq { const float* q; int64_t nq, k, nprobe; float scale, bias; const uint32_t* allow; };
struct ProbedOut { int64_t* idx; float* score; int64_t* probes; };

// The refusals that need no lock, then the lock and the partition's state: all before any device call.
std::unique_lock<std::mutex> enter_probed(clipgpu_index* ix, const ProbedReq& r, const ProbedOut& o) {
  if (!ix || !r.q || !o.idx || !o.score) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (r.nq <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (r.k < 1 || r.k > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k must be in 1.." + std::to_string(CLIPGPU_TOPK_MAX) +
                                           " (clipgpu_similarity gives the whole matrix)");
  if (r.nprobe < 1 || r.nprobe > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "nprobe must be in 1.." + std::to_string(CLIPGPU_TOPK_MAX) + ", got " +
                                           std::to_string(r.nprobe));
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->pt_C == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "the index has no partition (clipgpu_index_partition)");
  if (ix->pt_stale)
    throw ClipErr(CLIPGPU_ERR_INVALID, "the partition is stale: rows were added, replaced or cleared since "
                                       "clipgpu_index_partition (call it again)");
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

// Searches the device rows r.q on `s` under one mask into the device buffers of `o`, in chunks sized so that
// the workspace holds every block's k entries.  Per chunk: the coarse search of the centroid copy (launch_topk
// into pt_coarse; it has finished with the workspace before the probe kernel starts, by stream order), the
// probe kernel, the merge.  Nothing here synchronises.
void probed_on(clipgpu_index* ix, const ProbedReq& r, const uint32_t* mask, const ProbedOut& o, hipStream_t s) {
  const int C = (int)ix->pt_C, k = (int)r.k, E = (int)ix->E;
  const int np = (int)std::min<int64_t>(r.nprobe, C);  // the lists a query reads
  const long ws_entries = (long)ix->ws_blocks * 64 * kTopkMax;
  // the parts of a list: enough blocks to fill the GPU, no more parts than the longest list has tiles
  const long tiles = std::max<long>(1, (ix->pt_longest + 15) / 16);
  const long rows0 = std::min<int64_t>(kQueryChunk, r.nq);
  long S = std::min(tiles, std::max(1L, (kNarrowSpans + rows0 * np - 1) / (rows0 * np)));
  if (g_probe_parts.load() > 0) S = g_probe_parts.load();
  S = std::max(1L, std::min(S, std::min(65535L / np, ws_entries / ((long)np * k))));
  long chunk = std::min<long>(kQueryChunk, ws_entries / ((long)np * S * k));
  if (g_probe_chunk.load() > 0) chunk = std::min<long>(chunk, g_probe_chunk.load());
  if (o.probes && np < r.nprobe) HIP_CHECK(hipMemsetAsync(o.probes, 0xff, (size_t)r.nq * r.nprobe * 8, s));  // -1
  for (int64_t q0 = 0; q0 < r.nq; q0 += chunk) {
    const int rows = (int)std::min<int64_t>(chunk, r.nq - q0);
    const float* q = r.q + q0 * E;
    const TopkPlan p = topk_plan(C, rows, ix->ws_blocks);
    HIP_CHECK(launch_topk({q, rows, ix->pt_cen, TOPK_GAL_F32, C, E, 1.f, 0.f, np, p, ix->d_ws, nullptr, coarse_idx(ix),
                           coarse_score(ix), TOPK_PROBS_NONE, nullptr, 0, nullptr, nullptr, s}));
    if (o.probes)
      HIP_CHECK(hipMemcpy2DAsync(o.probes + q0 * r.nprobe, (size_t)r.nprobe * 8, coarse_idx(ix), (size_t)np * 8,
                                 (size_t)np * 8, rows, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(launch_probe({q, rows, ix->gallery, ix->dtype, (int)ix->size, E, r.scale, r.bias, k, coarse_idx(ix), np,
                            (int)S, (const int32_t*)ix->pt_off, (const int32_t*)ix->pt_ids, mask, ix->d_ws, s}));
    HIP_CHECK(launch_topk_merge(ix->d_ws, rows, np * (int)S, k, o.idx + q0 * k, o.score + q0 * k, s));
  }
  mark_last(ix, s);
}

int probed_device(clipgpu_index* ix, const ProbedReq& r, const ProbedOut& o, hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_probed(ix, r, o);
    order_after_last(ix, s);
    probed_on(ix, r, build_mask(ix, r.allow, s), o, s);
  });
}

int probed_host(clipgpu_index* ix, const ProbedReq& r, const ProbedOut& o) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_probed(ix, r, o);
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    const ProbedOut st = {ix->st_idx, ix->st_score, o.probes ? coarse_probes(ix) : nullptr};
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
      const ProbedReq c = {ix->st_q, std::min(kQueryChunk, r.nq - q0), r.k, r.nprobe, r.scale, r.bias, nullptr};
      HIP_CHECK(copy_h2d(ix->st_q, r.q + q0 * ix->E, (size_t)c.nq * ix->E * 4));
      probed_on(ix, c, mask, st, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(o.idx + q0 * r.k, st.idx, (size_t)c.nq * r.k * 8));
      HIP_CHECK(copy_d2h(o.score + q0 * r.k, st.score, (size_t)c.nq * r.k * 4));
      if (st.probes) HIP_CHECK(copy_d2h(o.probes + q0 * r.nprobe, st.probes, (size_t)c.nq * r.nprobe * 8));
    }
  });
}

// ---- int8 codes and the coded search (kernels/codes.hip) --------------------------------------------------
// The regions of cd_work: the staged codes and scales of a chunk of queries, the chunk's merged candidates and
// their coarse scores, and the candidates as the lists the probe kernel reads.
struct CodesWork { int8_t* qc; float* qs; int64_t* cand; float* coarse; int32_t* ids; int32_t* off; int64_t* lists; };
size_t carve_codes(const clipgpu_index* ix, CodesWork* w) {
  size_t off = 0, chunk = (size_t)kQueryChunk;
  char* base = ix->cd_work;
  CodesWork c;
  c.qc = carve<int8_t>(base, off, chunk * ix->cd_Ep);
  c.qs = carve<float>(base, off, chunk * 4);
  c.cand = carve<int64_t>(base, off, chunk * kTopkMax * 8);
  c.coarse = carve<float>(base, off, chunk * kTopkMax * 4);
  c.ids = carve<int32_t>(base, off, chunk * kTopkMax * 4);
  c.off = carve<int32_t>(base, off, (2 * chunk + 1) * 4);
  c.lists = carve<int64_t>(base, off, chunk * 8);
  if (w) *w = c;
  return off;
}

void free_codes(clipgpu_index* ix) {
  if (ix->cd_codes) (void)hipFree(ix->cd_codes);
  if (ix->cd_scale) (void)hipFree(ix->cd_scale);
  if (ix->cd_work) (void)hipFree(ix->cd_work);
  ix->cd_codes = nullptr;
  ix->cd_scale = nullptr;
  ix->cd_work = nullptr;
}

// Codes rows ids[0 .. n) (device ids) or [first, first + n) of the gallery on `s`, behind the write of those
// rows on the same stream.  Nothing if the index has no codes.
void code_rows(clipgpu_index* ix, const int64_t* d_ids, int64_t first, int64_t n, hipStream_t s) {
  if (!ix->cd_codes || n <= 0) return;
  HIP_CHECK(launch_codes_quant({ix->gallery, ix->dtype, (long)n, (int)ix->E, (int)ix->cd_Ep, d_ids, (long)first,
                                ix->cd_codes, ix->cd_scale, s}));
}

// One coded search call.  q, allow and the outputs: device pointers for coded_on and coded_device, host pointers
// for coded_host.  cand, coarse: [nq][refine] or NULL.
struct CodedReq { const float* q; int64_t nq, k, refine; float scale, bias; const uint32_t* allow; };
struct CodedOut { int64_t* idx; float* score; int64_t* cand; float* coarse; };

// The refusals that need no lock, then the lock and the codes: all before any device call.
std::unique_lock<std::mutex> enter_coded(clipgpu_index* ix, const CodedReq& r, const CodedOut& o) {
  if (!ix || !r.q || !o.idx || !o.score) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (r.nq <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (r.k < 1 || r.k > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k must be in 1.." + std::to_string(CLIPGPU_TOPK_MAX) +
                                           " (clipgpu_similarity gives the whole matrix)");
  if (r.refine < r.k || r.refine > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "refine must be in k.." + std::to_string(CLIPGPU_TOPK_MAX) + ", got " +
                                           std::to_string(r.refine));
  std::unique_lock<std::mutex> lk(ix->mu);
  if (!ix->cd_codes) throw ClipErr(CLIPGPU_ERR_INVALID, "the index has no codes (clipgpu_index_enable_codes)");
  if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // an empty gallery
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

// Searches the device rows r.q on `s` under one mask into the device buffers of `o`, in chunks of kQueryChunk
// rows.  Per chunk, the coarse stage: the queries' codes, the scan (the search's route and span cut) and the merge
// with k = refine into cd_work; then the re-rank: the candidates as lists, the probe kernel over list 2q for
// query q (the candidates passed the mask already), the merge.  Stream order keeps the two users of the
// workspace apart.  Nothing here synchronises.
void coded_on(clipgpu_index* ix, const CodedReq& r, const uint32_t* mask, const CodedOut& o, hipStream_t s) {
  const int E = (int)ix->E, k = (int)r.k, R = (int)r.refine, stage = g_codes_stage.load();
  const long ws_entries = (long)ix->ws_blocks * 64 * kTopkMax;
  CodesWork w;
  carve_codes(ix, &w);
  for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
    const int rows = (int)std::min(kQueryChunk, r.nq - q0);
    const float* q = r.q + q0 * E;
    if (stage != 2) {
      HIP_CHECK(launch_codes_quant({q, TOPK_GAL_F32, rows, E, (int)ix->cd_Ep, nullptr, 0, w.qc, w.qs, s}));
      const TopkPlan p = topk_plan(ix->size, rows, ix->ws_blocks);
      HIP_CHECK(launch_codes_scan({w.qc, rows, ix->cd_codes, ix->cd_scale, (int)ix->size, (int)ix->cd_Ep, r.scale < 0.f,
                                   R, p, ix->d_ws, mask, s}));
      HIP_CHECK(launch_topk_merge(ix->d_ws, rows, p.n_spans, R, w.cand, w.coarse, s));
      if (o.cand)
        HIP_CHECK(hipMemcpyAsync(o.cand + q0 * R, w.cand, (size_t)rows * R * 8, hipMemcpyDeviceToDevice, s));
      if (o.coarse)
        HIP_CHECK(hipMemcpyAsync(o.coarse + q0 * R, w.coarse, (size_t)rows * R * 4, hipMemcpyDeviceToDevice, s));
    }
    if (stage != 1) {
      HIP_CHECK(launch_codes_lists(w.cand, rows, R, w.ids, w.off, w.lists, s));
      // the parts of a candidate list, as probed_on chooses them: enough blocks to fill the GPU, no more than tiles
      long S = std::min<long>((R + 15) / 16, std::max(1L, (kNarrowSpans + rows - 1L) / rows));
      if (g_probe_parts.load() > 0) S = g_probe_parts.load();
      S = std::max(1L, std::min(S, std::min(65535L, ws_entries / ((long)rows * k))));
      HIP_CHECK(launch_probe({q, rows, ix->gallery, ix->dtype, (int)ix->size, E, r.scale, r.bias, k, w.lists, 1, (int)S,
                              w.off, w.ids, nullptr, ix->d_ws, s}));
      HIP_CHECK(launch_topk_merge(ix->d_ws, rows, (int)S, k, o.idx + q0 * k, o.score + q0 * k, s));
    }
  }
  mark_last(ix, s);
}

int coded_device(clipgpu_index* ix, const CodedReq& r, const CodedOut& o, hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_coded(ix, r, o);
    order_after_last(ix, s);
    coded_on(ix, r, build_mask(ix, r.allow, s), o, s);
  });
}

int coded_host(clipgpu_index* ix, const CodedReq& r, const CodedOut& o) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_coded(ix, r, o);
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    CodesWork w;
    carve_codes(ix, &w);
    const CodedOut st = {ix->st_idx, ix->st_score, nullptr, nullptr};  // the candidates are read where the merge leaves them
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
      const CodedReq c = {ix->st_q, std::min(kQueryChunk, r.nq - q0), r.k, r.refine, r.scale, r.bias, nullptr};
      HIP_CHECK(copy_h2d(ix->st_q, r.q + q0 * ix->E, (size_t)c.nq * ix->E * 4));
      coded_on(ix, c, mask, st, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(o.idx + q0 * r.k, st.idx, (size_t)c.nq * r.k * 8));
      HIP_CHECK(copy_d2h(o.score + q0 * r.k, st.score, (size_t)c.nq * r.k * 4));
      if (o.cand) HIP_CHECK(copy_d2h(o.cand + q0 * r.refine, w.cand, (size_t)c.nq * r.refine * 8));
      if (o.coarse) HIP_CHECK(copy_d2h(o.coarse + q0 * r.refine, w.coarse, (size_t)c.nq * r.refine * 4));
    }
  });
}

// ---- deep search (kernels/deep.hip) -----------------------------------------------------------------------
// One call, as SearchReq / SearchOut; passes: int32 [nq] or NULL.
struct DeepReq { const float* q; int64_t nq, k; float scale, bias; const uint32_t* allow; };
struct DeepOut { int64_t* idx; float* score; int32_t* passes; };

// The refusals that need no lock; then as enter_search.
std::unique_lock<std::mutex> enter_deep(clipgpu_index* ix, const DeepReq& r, const DeepOut& o) {
  if (!ix || !r.q || !o.idx || !o.score) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (r.nq <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (r.k < 1 || r.k > CLIPGPU_DEEP_K_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k must be in 1.." + std::to_string(CLIPGPU_DEEP_K_MAX) + ", got " +
                                           std::to_string(r.k));
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // an empty gallery
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

// The deep search's work area: the chunk's device state (deep_carve) and, behind it, the host form's staged
// indices, scores and pass counts (`st`).  Allocated at the first deep search; a failed allocation is
// CLIPGPU_ERR_DEVICE and leaves the handle without the area, usable.  Callers hold the mutex.
DeepWork deep_buffers(clipgpu_index* ix, DeepOut* st) {
  DeepWork w;
  size_t off = deep_carve(nullptr, &w);
  const size_t slots = (size_t)kDeepChunk * kDeepKMax;
  off += align256(slots * 8) + align256(slots * 4) + align256((size_t)kDeepChunk * 4);
  if (!ix->dp_work) HIP_CHECK(hipMalloc((void**)&ix->dp_work, off));
  off = deep_carve(ix->dp_work, &w);
  st->idx = carve<int64_t>(ix->dp_work, off, slots * 8);
  st->score = carve<float>(ix->dp_work, off, slots * 4);
  st->passes = carve<int32_t>(ix->dp_work, off, (size_t)kDeepChunk * 4);
  return w;
}

// Searches the device rows r.q in chunks of kQueryChunk rows on `s`, all under one mask, into the device
// buffers of `o`: per chunk the fixed launch sequence of launch_deep, nothing read back.
void deep_on(clipgpu_index* ix, const DeepReq& r, const uint32_t* mask, const DeepWork& w, const DeepOut& o,
             hipStream_t s) {
  static_assert(kQueryChunk == kDeepChunk, "a chunk's state holds kDeepChunk queries");
  for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
    const int rows = (int)std::min(kQueryChunk, r.nq - q0);
    const TopkPlan p = topk_plan(ix->size, rows, ix->ws_blocks);  // the search's route and span cut
    HIP_CHECK(launch_deep({r.q + q0 * ix->E, rows, ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, r.scale, r.bias,
                           (int)r.k, p, mask, w, o.idx + q0 * r.k, o.score + q0 * r.k,
                           o.passes ? o.passes + q0 : nullptr, s}));
  }
  mark_last(ix, s);
}

int deep_device(clipgpu_index* ix, const DeepReq& r, const DeepOut& o, hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_deep(ix, r, o);
    DeepOut st;
    const DeepWork w = deep_buffers(ix, &st);
    order_after_last(ix, s);
    deep_on(ix, r, build_mask(ix, r.allow, s), w, o, s);
  });
}

int deep_host(clipgpu_index* ix, const DeepReq& r, const DeepOut& o) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_deep(ix, r, o);
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    DeepOut st;
    const DeepWork w = deep_buffers(ix, &st);
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    if (!o.passes) st.passes = nullptr;
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
      const DeepReq c = {ix->st_q, std::min(kQueryChunk, r.nq - q0), r.k, r.scale, r.bias, nullptr};
      HIP_CHECK(copy_h2d(ix->st_q, r.q + q0 * ix->E, (size_t)c.nq * ix->E * 4));
      deep_on(ix, c, mask, w, st, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(o.idx + q0 * r.k, st.idx, (size_t)c.nq * r.k * 8));
      HIP_CHECK(copy_d2h(o.score + q0 * r.k, st.score, (size_t)c.nq * r.k * 4));
      if (st.passes) HIP_CHECK(copy_d2h(o.passes + q0, st.passes, (size_t)c.nq * 4));
    }
  });
}

// ---- compound queries (kernels/compound.hip) --------------------------------------------------------------
// One call.  Host form: terms [T][E] and lims int64 [nq + 1] on the host, checked here.  Device form: d_terms and
// d_lims (int32) on the device, max_terms the caller's bound on a group's size (the device clamps to it).
struct CompoundReq { const float* terms; int64_t T, nq, k; int op; float scale, bias; const uint32_t* allow; };

// The regions of cp_work: a chunk's offsets, its staged terms (host form) and its padded tile rows.
struct CompoundWork { int32_t* lims; float* terms; float* tiles; };
constexpr size_t kCompoundRows = (size_t)kQueryChunk * kCompoundTermsMax;  // most terms, and tile rows, of a chunk
// Allocated at the first compound search (grow: the owner of the handle's lazy buffers) and kept until the handle
// is destroyed; a failed allocation is CLIPGPU_ERR_DEVICE and leaves the handle without the area, usable.
// Callers hold the mutex.
CompoundWork compound_buffers(clipgpu_index* ix) {
  const size_t rows_bytes = align256(kCompoundRows * ix->E * 4);
  grow(ix->cp_work, ix->cp_work_n, 1, 2048 + 2 * rows_bytes);
  CompoundWork w;
  w.lims = (int32_t*)ix->cp_work;  // kQueryChunk + 1 offsets: 1028 bytes
  w.terms = (float*)(ix->cp_work + 2048);
  w.tiles = (float*)(ix->cp_work + 2048 + rows_bytes);
  return w;
}

// The refusals that need no lock, in the order the header lists them; then as enter_search.
std::unique_lock<std::mutex> enter_compound(clipgpu_index* ix, const CompoundReq& r, bool null_arg) {
  if (!ix || null_arg) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (r.nq <= 0 || r.T <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (r.k < 1 || r.k > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k must be in 1.." + std::to_string(CLIPGPU_TOPK_MAX) + ", got " +
                                           std::to_string(r.k));
  if (r.op != CLIPGPU_COMPOUND_MIN && r.op != CLIPGPU_COMPOUND_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "op must be CLIPGPU_COMPOUND_MIN (0) or CLIPGPU_COMPOUND_MAX (1), got " +
                                           std::to_string(r.op));
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // an empty gallery
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

std::string terms_range() { return "1.." + std::to_string(CLIPGPU_COMPOUND_TERMS_MAX) + " terms (CLIPGPU_COMPOUND_TERMS_MAX)"; }

// One chunk of `rows` compound queries on `s`: d_lims (device int32 [rows + 1]) into d_terms [T][E], slot width
// G.  The gather pads the tile rows into cp_work, the phase 1 fills the search workspace, the merge writes the
// result.  Stream order keeps the chunks of a call, which share both, apart.
void compound_chunk(clipgpu_index* ix, const CompoundReq& r, const float* d_terms, const int32_t* d_lims, int rows,
                    int G, const uint32_t* mask, float* tiles, int64_t* d_idx, float* d_score, hipStream_t s) {
  HIP_CHECK(launch_compound_gather(d_terms, (long)r.T, d_lims, rows, G, (int)ix->E, tiles, s));
  const TopkPlan p = compound_plan(ix->size, rows, G, ix->ws_blocks);
  HIP_CHECK(launch_compound({tiles, rows, G, r.op, ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, r.scale, r.bias,
                             (int)r.k, p, ix->d_ws, mask, s}));
  HIP_CHECK(launch_topk_merge(ix->d_ws, rows, p.n_spans, (int)r.k, d_idx, d_score, s));
}

int compound_device(clipgpu_index* ix, const CompoundReq& r, const int32_t* d_lims, int64_t max_terms, int64_t* d_idx,
                    float* d_score, hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_compound(ix, r, !r.terms || !d_lims || !d_idx || !d_score);
    if (max_terms < 1 || max_terms > CLIPGPU_COMPOUND_TERMS_MAX)
      throw ClipErr(CLIPGPU_ERR_INVALID, "max_terms: a group has " + terms_range() + ", got " + std::to_string(max_terms));
    if (r.T > INT32_MAX) throw ClipErr(CLIPGPU_ERR_INVALID, "too many terms (d_lims holds int32)");
    if ((uintptr_t)r.terms & 15) throw ClipErr(CLIPGPU_ERR_INVALID, "d_terms must be 16-byte aligned");
    const CompoundWork w = compound_buffers(ix);
    order_after_last(ix, s);
    const uint32_t* mask = build_mask(ix, r.allow, s);
    const int G = compound_width((int)max_terms);
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk)
      compound_chunk(ix, r, r.terms, d_lims + q0, (int)std::min(kQueryChunk, r.nq - q0), G, mask, w.tiles,
                     d_idx + q0 * r.k, d_score + q0 * r.k, s);
    mark_last(ix, s);
  });
}

int compound_host(clipgpu_index* ix, const CompoundReq& r, const int64_t* lims, int64_t* out_idx, float* out_score) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_compound(ix, r, !r.terms || !lims || !out_idx || !out_score);
    if (lims[0] != 0) throw ClipErr(CLIPGPU_ERR_INVALID, "lims must start at 0, got " + std::to_string(lims[0]));
    for (int64_t q = 0; q < r.nq; ++q) {
      const int64_t n = lims[q + 1] - lims[q];
      if (n < 0) throw ClipErr(CLIPGPU_ERR_INVALID, "lims must be ascending (at query " + std::to_string(q) + ")");
      if (n < 1 || n > CLIPGPU_COMPOUND_TERMS_MAX)
        throw ClipErr(CLIPGPU_ERR_INVALID, "a query has " + terms_range() + ", query " + std::to_string(q) + " has " +
                                               std::to_string(n));
    }
    if (lims[r.nq] != r.T)
      throw ClipErr(CLIPGPU_ERR_INVALID, "lims must end at the number of terms, " + std::to_string(r.T) + ", got " +
                                             std::to_string(lims[r.nq]));
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    const CompoundWork w = compound_buffers(ix);
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    std::vector<int32_t> rel((size_t)kQueryChunk + 1);
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
      // the chunk's terms and its offsets from the first of them; its slot width from its own largest group
      const int rows = (int)std::min(kQueryChunk, r.nq - q0);
      int largest = 1;
      for (int q = 0; q <= rows; ++q) rel[q] = (int32_t)(lims[q0 + q] - lims[q0]);
      for (int q = 0; q < rows; ++q) largest = std::max(largest, rel[q + 1] - rel[q]);
      CompoundReq c = r;
      c.T = rel[rows];
      HIP_CHECK(copy_h2d(w.lims, rel.data(), (size_t)(rows + 1) * 4));
      HIP_CHECK(copy_h2d(w.terms, r.terms + lims[q0] * ix->E, (size_t)c.T * ix->E * 4));
      compound_chunk(ix, c, w.terms, w.lims, rows, compound_width(largest), mask, w.tiles, ix->st_idx, ix->st_score,
                     ix->stream);
      mark_last(ix, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(out_idx + q0 * r.k, ix->st_idx, (size_t)rows * r.k * 8));
      HIP_CHECK(copy_d2h(out_score + q0 * r.k, ix->st_score, (size_t)rows * r.k * 4));
    }
  });
}

// ---- group labels and the grouped search (kernels/grouped.hip) ----------------------------------------------
size_t group_label_bytes(const clipgpu_index* ix) { return align256((size_t)ix->capacity * 4); }
int64_t* staged_groups(clipgpu_index* ix) { return (int64_t*)(ix->gp_labels + group_label_bytes(ix)); }

// The labels, allocated and filled with "ungrouped" at the first use (synchronous, once per handle); a failed
// allocation is CLIPGPU_ERR_DEVICE and leaves the handle without them, usable.  Callers hold the mutex.
uint32_t* group_labels(clipgpu_index* ix) {
  if (!ix->gp_labels) {
    char* p = nullptr;
    HIP_CHECK(hipMalloc((void**)&p, group_label_bytes(ix) + (size_t)kQueryChunk * kTopkMax * 8));
    hipError_t err = launch_group_fill((uint32_t*)p, 0, (long)ix->capacity, ix->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ix->stream);
    if (err != hipSuccess) {
      (void)hipFree(p);
      HIP_CHECK(err);
    }
    ix->gp_labels = p;
  }
  return (uint32_t*)ix->gp_labels;
}

struct GroupedOut { int64_t* idx; float* score; int64_t* group; };

// Searches the device rows r.q in chunks of kQueryChunk rows on `s`, all under one mask, into the device buffers
// of `o`.  The span cut is the compound search's at width 1: one-wave blocks over (query tiles, spans), such that
// the workspace holds a chunk's rows.
void grouped_on(clipgpu_index* ix, const SearchReq& r, const uint32_t* mask, const uint32_t* labels, const GroupedOut& o,
                hipStream_t s) {
  for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
    const int rows = (int)std::min(kQueryChunk, r.nq - q0);
    const TopkPlan p = compound_plan(ix->size, rows, 1, ix->ws_blocks);
    HIP_CHECK(launch_grouped({r.q + q0 * ix->E, rows, ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, r.scale, r.bias,
                              (int)r.k, p, ix->d_ws, mask, labels, o.idx + q0 * r.k, o.score + q0 * r.k,
                              o.group ? o.group + q0 * r.k : nullptr, s}));
  }
  mark_last(ix, s);
}

int grouped_device(clipgpu_index* ix, const SearchReq& r, const GroupedOut& o, hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_search(ix, r, {o.idx, o.score, nullptr, nullptr});
    if ((uintptr_t)r.q & 15) throw ClipErr(CLIPGPU_ERR_INVALID, "d_queries must be 16-byte aligned");
    const uint32_t* labels = group_labels(ix);
    order_after_last(ix, s);
    grouped_on(ix, r, build_mask(ix, r.allow, s), labels, o, s);
  });
}

int grouped_host(clipgpu_index* ix, const SearchReq& r, const GroupedOut& o) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_search(ix, r, {o.idx, o.score, nullptr, nullptr});
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    const uint32_t* labels = group_labels(ix);
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    const GroupedOut st = {ix->st_idx, ix->st_score, o.group ? staged_groups(ix) : nullptr};
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
      const SearchReq c = {ix->st_q, std::min(kQueryChunk, r.nq - q0), r.k, r.scale, r.bias, TOPK_PROBS_NONE, nullptr};
      HIP_CHECK(copy_h2d(ix->st_q, r.q + q0 * ix->E, (size_t)c.nq * ix->E * 4));
      grouped_on(ix, c, mask, labels, st, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(o.idx + q0 * r.k, st.idx, (size_t)c.nq * r.k * 8));
      HIP_CHECK(copy_d2h(o.score + q0 * r.k, st.score, (size_t)c.nq * r.k * 4));
      if (st.group) HIP_CHECK(copy_d2h(o.group + q0 * r.k, st.group, (size_t)c.nq * r.k * 8));
    }
  });
}

// ---- the diversified search (kernels/diverse.hip) ------------------------------------------------------------
// What is asked beyond a SearchReq, and the optional pool outputs [nq][pool] (device or host, as the form's).
struct DiverseReq { int64_t pool; float diversity; int64_t* pool_idx; float* pool_score; };
// The regions of dv_work: a chunk's pool [kQueryChunk][kTopkMax] and its Gram matrices [kQueryChunk][P][P].
struct DiverseWork { int64_t* idx; float* score; float* gram; };
constexpr size_t kDiversePool = (size_t)kQueryChunk * kTopkMax;

// The refusals of the pool and the diversity, after enter_search's; then the work area for pools of d.pool: grow,
// the owner of the handle's lazy buffers, which frees a smaller area -- so a search in flight is waited for first.
// A failed allocation is CLIPGPU_ERR_DEVICE and leaves the handle without the area, usable.  Callers hold the mutex.
DiverseWork diverse_buffers(clipgpu_index* ix, const SearchReq& r, const DiverseReq& d) {
  const std::string range = "1.." + std::to_string(CLIPGPU_TOPK_MAX);
  if (d.pool < 1 || d.pool > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "pool must be in " + range + ", got " + std::to_string(d.pool));
  if (r.k > d.pool)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k <= pool is required (pool in " + range + "), got k " + std::to_string(r.k) +
                                           ", pool " + std::to_string(d.pool));
  if (!(d.diversity >= 0.0f && d.diversity <= 1.0f))
    throw ClipErr(CLIPGPU_ERR_INVALID, "diversity must be in [0, 1], got " + std::to_string(d.diversity));
  if ((d.pool_idx == nullptr) != (d.pool_score == nullptr))
    throw ClipErr(CLIPGPU_ERR_INVALID, "the pool outputs come as a pair: both or neither");
  if (d.pool > ix->dv_work_n && ix->dv_work) HIP_CHECK(hipEventSynchronize(ix->done));
  grow(ix->dv_work, ix->dv_work_n, d.pool, kDiversePool * 12 + (size_t)kQueryChunk * d.pool * d.pool * 4);
  DiverseWork w;
  w.idx = (int64_t*)ix->dv_work;
  w.score = (float*)(ix->dv_work + kDiversePool * 8);
  w.gram = (float*)(ix->dv_work + kDiversePool * 12);
  return w;
}

// One chunk of `rows` device queries on `s`: the pool by the search's own launch (into pool_idx / pool_score,
// [rows][pool]), then the re-ranking into d_idx / d_score [rows][k].  Stream order keeps the chunks of a call,
// which share the Gram area, apart.
void diverse_chunk(clipgpu_index* ix, const SearchReq& r, const float* d_q, int rows, const DiverseReq& d,
                   const uint32_t* mask, int64_t* pool_idx, float* pool_score, float* gram, int64_t* d_idx,
                   float* d_score, hipStream_t s) {
  search_on(ix, {d_q, rows, d.pool, r.scale, r.bias, TOPK_PROBS_NONE, nullptr}, mask, {pool_idx, pool_score, nullptr, nullptr},
            s);
  HIP_CHECK(launch_diverse({ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, rows, (int)d.pool, (int)r.k, r.scale, r.bias,
                            d.diversity, pool_idx, pool_score, gram, d_idx, d_score, s}));
  mark_last(ix, s);
}

int diverse_device(clipgpu_index* ix, const SearchReq& r, const DiverseReq& d, int64_t* d_idx, float* d_score,
                   hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_search(ix, r, {d_idx, d_score, nullptr, nullptr});
    const DiverseWork w = diverse_buffers(ix, r, d);
    order_after_last(ix, s);
    const uint32_t* mask = build_mask(ix, r.allow, s);
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk)  // the caller's pool buffers hold every chunk, the area one
      diverse_chunk(ix, r, r.q + q0 * ix->E, (int)std::min(kQueryChunk, r.nq - q0), d, mask,
                    d.pool_idx ? d.pool_idx + q0 * d.pool : w.idx, d.pool_score ? d.pool_score + q0 * d.pool : w.score,
                    w.gram, d_idx + q0 * r.k, d_score + q0 * r.k, s);
  });
}

int diverse_host(clipgpu_index* ix, const SearchReq& r, const DiverseReq& d, int64_t* out_idx, float* out_score) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_search(ix, r, {out_idx, out_score, nullptr, nullptr});
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers and the filter area are free
    const DiverseWork w = diverse_buffers(ix, r, d);
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    for (int64_t q0 = 0; q0 < r.nq; q0 += kQueryChunk) {
      const int64_t rows = std::min(kQueryChunk, r.nq - q0);
      HIP_CHECK(copy_h2d(ix->st_q, r.q + q0 * ix->E, (size_t)rows * ix->E * 4));
      diverse_chunk(ix, r, ix->st_q, (int)rows, d, mask, w.idx, w.score, w.gram, ix->st_idx, ix->st_score, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(out_idx + q0 * r.k, ix->st_idx, (size_t)rows * r.k * 8));
      HIP_CHECK(copy_d2h(out_score + q0 * r.k, ix->st_score, (size_t)rows * r.k * 4));
      if (d.pool_idx) {
        HIP_CHECK(copy_d2h(d.pool_idx + q0 * d.pool, w.idx, (size_t)rows * d.pool * 8));
        HIP_CHECK(copy_d2h(d.pool_score + q0 * d.pool, w.score, (size_t)rows * d.pool * 4));
      }
    }
  });
}

// ---- neighbours of stored rows and the k-NN graph (kernels/knn.hip) ------------------------------------------
// ids [n] (device for the device form, host for the host form), or NULL: every slot, n == size, graph semantics.
struct KnnReq { const int64_t* ids; int64_t n, k; float scale, bias; const uint32_t* allow; };
constexpr int64_t kKnnPiece = 8192;  // query rows the host form stages at once: 128 panels
// The host form's area: a piece's ids int64 [kKnnPiece], indices int64 and scores f32 [kKnnPiece][kTopkMax].
struct KnnWork { int64_t* ids; int64_t* idx; float* score; };

// host: r.ids are host ids, refused here if one is out of range, before any device call.
std::unique_lock<std::mutex> enter_knn(clipgpu_index* ix, const KnnReq& r, const void* idx, const void* score, bool host) {
  if (!ix || !idx || !score) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (r.n <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  if (r.k < 1 || r.k > CLIPGPU_TOPK_MAX)
    throw ClipErr(CLIPGPU_ERR_INVALID, "k must be in 1.." + std::to_string(CLIPGPU_TOPK_MAX) +
                                           " (clipgpu_index_search_deep searches deeper, for a query given as a row)");
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->size == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // an empty gallery
  if (!r.ids && r.n != ix->size)
    throw ClipErr(CLIPGPU_ERR_INVALID, "without ids n must be the index's size, " + std::to_string(ix->size) + ", got " +
                                           std::to_string(r.n));
  if (host && r.ids) check_ids_in_range(ix, r.ids, r.n);
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

// Query rows [r0, r0 + rows) of a call on `s`, into d_idx / d_score [rows][k]: as many launches as the search
// workspace asks for at the call's span cut p, in stream order (they share it).  d_ids: the rows' ids, or NULL.
// The validity bits of a query row: the filter itself for the graph, the live bits alone for named rows.
void knn_on(clipgpu_index* ix, const KnnReq& r, const TopkPlan& p, const int64_t* d_ids, int64_t r0, int64_t rows,
            const uint32_t* mask, int64_t* d_idx, float* d_score, hipStream_t s) {
  const uint32_t* qvalid = !r.ids ? mask : ix->n_dead ? ix->d_live : nullptr;
  const int64_t step = knn_launch_rows(p, (int)r.k, ix->ws_blocks);
  for (int64_t q0 = 0; q0 < rows; q0 += step) {
    const int m = (int)std::min(step, rows - q0);
    HIP_CHECK(launch_knn({ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, d_ids ? d_ids + q0 : nullptr, r0 + q0, m,
                          (int)r.k, r.scale, r.bias, p, ix->d_ws, (long)ix->ws_blocks * 64 * kTopkMax, mask, qvalid,
                          d_idx + q0 * r.k, d_score + q0 * r.k, s}));
  }
  mark_last(ix, s);
}

int knn_device(clipgpu_index* ix, const KnnReq& r, int64_t* d_idx, float* d_score, hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_knn(ix, r, d_idx, d_score, false);
    order_after_last(ix, s);
    const uint32_t* mask = build_mask(ix, r.allow, s);
    knn_on(ix, r, knn_plan(ix->size, (r.n + 63) / 64, ix->ws_blocks), r.ids, 0, r.n, mask, d_idx, d_score, s);
  });
}

int knn_host(clipgpu_index* ix, const KnnReq& r, int64_t* out_idx, float* out_score) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_knn(ix, r, out_idx, out_score, true);
    HIP_CHECK(hipEventSynchronize(ix->done));  // the filter area and the staging area are free
    grow(ix->kn_work, ix->kn_work_n, kKnnPiece, (size_t)kKnnPiece * (8 + (size_t)kTopkMax * 12));
    const KnnWork w = {(int64_t*)ix->kn_work, (int64_t*)(ix->kn_work + kKnnPiece * 8),
                       (float*)(ix->kn_work + kKnnPiece * 8 + kKnnPiece * kTopkMax * 8)};
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    const TopkPlan p = knn_plan(ix->size, (r.n + 63) / 64, ix->ws_blocks);
    for (int64_t r0 = 0; r0 < r.n; r0 += kKnnPiece) {
      const int64_t rows = std::min(kKnnPiece, r.n - r0);
      if (r.ids) HIP_CHECK(copy_h2d(w.ids, r.ids + r0, (size_t)rows * 8));
      knn_on(ix, r, p, r.ids ? w.ids : nullptr, r0, rows, mask, w.idx, w.score, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(out_idx + r0 * r.k, w.idx, (size_t)rows * r.k * 8));
      HIP_CHECK(copy_d2h(out_score + r0 * r.k, w.score, (size_t)rows * r.k * 4));
    }
  });
}

// ---- duplicate groups (kernels/components.hip) ----------------------------------------------------------------
struct CcReq { float thr, scale, bias; const uint32_t* allow; bool to_groups; };
// The regions of cc_work.
struct CcBuf { int32_t* parent; int32_t* label; uint32_t* count; };

// The refusals that need no lock and no device; then the lock and the handle's device.  An empty index is no error.
std::unique_lock<std::mutex> enter_components(clipgpu_index* ix, bool null_arg, const CcReq& r) {
  if (!ix || null_arg) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
  if (r.thr != r.thr) throw ClipErr(CLIPGPU_ERR_INVALID, "threshold must not be NaN");
  std::unique_lock<std::mutex> lk(ix->mu);
  HIP_CHECK(hipSetDevice(ix->device));
  return lk;
}

// Allocated at the first call; a failed allocation is CLIPGPU_ERR_DEVICE and leaves the handle without the
// buffer, usable.  Callers hold the mutex.
CcBuf components_buffers(clipgpu_index* ix) {
  const size_t slots = align256((size_t)ix->capacity * 4);
  if (!ix->cc_work) HIP_CHECK(hipMalloc((void**)&ix->cc_work, 2 * slots + 256));
  size_t off = 0;
  CcBuf b;
  b.parent = carve<int32_t>(ix->cc_work, off, slots);
  b.label = carve<int32_t>(ix->cc_work, off, slots);
  b.count = carve<uint32_t>(ix->cc_work, off, 4);
  return b;
}

// The three launches on `s` (ordered behind the handle's last operation by the caller) into device buffers.
void components_on(clipgpu_index* ix, const CcReq& r, const CcBuf& b, const uint32_t* mask, uint32_t* groups,
                   int32_t* d_label, uint32_t* d_count, hipStream_t s) {
  HIP_CHECK(launch_components({ix->gallery, ix->dtype, (int)ix->size, (int)ix->E, r.scale, r.bias, r.thr, mask, b.parent,
                               d_label, groups, d_count, s}));
  mark_last(ix, s);
}

int components_device(clipgpu_index* ix, const CcReq& r, int32_t* d_label, uint32_t* d_count, hipStream_t s) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_components(ix, !d_label && !r.to_groups, r);
    const CcBuf b = ix->size > 0 ? components_buffers(ix) : CcBuf{};  // an empty index: the count is zeroed, no more
    uint32_t* groups = r.to_groups && ix->size > 0 ? group_labels(ix) : nullptr;
    order_after_last(ix, s);
    const uint32_t* mask = ix->size > 0 ? build_mask(ix, r.allow, s) : nullptr;
    components_on(ix, r, b, mask, groups, d_label, d_count, s);
  });
}

int components_host(clipgpu_index* ix, const CcReq& r, int64_t* out_label, int64_t* out_count) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_components(ix, !out_label || !out_count, r);
    *out_count = 0;
    if (ix->size == 0) return;
    HIP_CHECK(hipEventSynchronize(ix->done));  // the filter area and the staged labels are free
    const CcBuf b = components_buffers(ix);
    uint32_t* groups = r.to_groups ? group_labels(ix) : nullptr;
    if (r.allow) HIP_CHECK(copy_h2d(ix->d_eff, r.allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, r.allow ? ix->d_eff : nullptr, ix->stream);
    components_on(ix, r, b, mask, groups, b.label, b.count, ix->stream);
    HIP_CHECK(hipStreamSynchronize(ix->stream));
    std::vector<int32_t> l((size_t)ix->size);
    uint32_t count = 0;
    HIP_CHECK(copy_d2h(l.data(), b.label, l.size() * 4));
    HIP_CHECK(copy_d2h(&count, b.count, 4));
    for (size_t i = 0; i < l.size(); ++i) out_label[i] = l[i];
    *out_count = count;
  });
}

}  // namespace

extern "C" {

int clipgpu_index_components(clipgpu_index* ix, float threshold, float logit_scale, float logit_bias,
                             const uint32_t* allow, int to_groups, int64_t* out_label, int64_t* out_count) {
  return components_host(ix, {threshold, logit_scale, logit_bias, allow, to_groups != 0}, out_label, out_count);
}

int clipgpu_index_components_device(clipgpu_index* ix, float threshold, float logit_scale, float logit_bias,
                                    const uint32_t* d_allow, int to_groups, int32_t* d_label, uint32_t* d_count,
                                    void* stream) {
  return components_device(ix, {threshold, logit_scale, logit_bias, d_allow, to_groups != 0}, d_label, d_count,
                           (hipStream_t)stream);
}

int clipgpu_index_neighbors(clipgpu_index* ix, const int64_t* ids, int64_t n, int64_t k, float logit_scale,
                            float logit_bias, const uint32_t* allow, int64_t* out_idx, float* out_score) {
  return knn_host(ix, {ids, n, k, logit_scale, logit_bias, allow}, out_idx, out_score);
}

int clipgpu_index_neighbors_device(clipgpu_index* ix, const int64_t* d_ids, int64_t n, int64_t k, float logit_scale,
                                   float logit_bias, const uint32_t* d_allow, int64_t* d_idx, float* d_score,
                                   void* stream) {
  return knn_device(ix, {d_ids, n, k, logit_scale, logit_bias, d_allow}, d_idx, d_score, (hipStream_t)stream);
}

int clipgpu_index_search_diverse(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, int64_t pool,
                                 float diversity, float logit_scale, float logit_bias, const uint32_t* allow,
                                 int64_t* out_idx, float* out_score, int64_t* out_pool_idx, float* out_pool_score) {
  return diverse_host(ix, {queries, nq, k, logit_scale, logit_bias, TOPK_PROBS_NONE, allow},
                      {pool, diversity, out_pool_idx, out_pool_score}, out_idx, out_score);
}

int clipgpu_index_search_diverse_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k, int64_t pool,
                                        float diversity, float logit_scale, float logit_bias, const uint32_t* d_allow,
                                        int64_t* d_idx, float* d_score, int64_t* d_pool_idx, float* d_pool_score,
                                        void* stream) {
  return diverse_device(ix, {d_queries, nq, k, logit_scale, logit_bias, TOPK_PROBS_NONE, d_allow},
                        {pool, diversity, d_pool_idx, d_pool_score}, d_idx, d_score, (hipStream_t)stream);
}

int clipgpu_index_set_groups(clipgpu_index* ix, const int64_t* ids, const int32_t* groups, int64_t n) {
  return guarded([&]() {
    check_ids(ix, ids, n);
    if (!groups && n > 0) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    check_ids_in_range(ix, ids, n);  // before any change and any device work
    for (int64_t i = 0; i < n; ++i)
      if (groups[i] < -1)
        throw ClipErr(CLIPGPU_ERR_INVALID, "a group label must be in 0..2147483647, or -1 for no group, got " +
                                               std::to_string(groups[i]));
    std::vector<int64_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) throw ClipErr(CLIPGPU_ERR_INVALID, "duplicate id");
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    uint32_t* labels = group_labels(ix);
    // the ids and, behind them, their labels go through the scratch, in pieces of at most 2^20 rows
    const int64_t piece = std::min<int64_t>(n, 1 << 20);
    char* d = (char*)scratch_bytes(ix, (size_t)piece * 12);
    for (int64_t r0 = 0; r0 < n; r0 += piece) {
      const int64_t m = std::min(piece, n - r0);
      HIP_CHECK(copy_h2d(d, ids + r0, (size_t)m * 8));
      HIP_CHECK(copy_h2d(d + piece * 8, groups + r0, (size_t)m * 4));
      HIP_CHECK(launch_group_set((const int64_t*)d, (const int32_t*)(d + piece * 8), (long)m, labels, (long)ix->size,
                                 ix->stream));
      HIP_CHECK(hipStreamSynchronize(ix->stream));
    }
    mark_last(ix, ix->stream);
  });
}

int clipgpu_index_groups(clipgpu_index* ix, int32_t* out) {
  return guarded([&]() {
    if (!ix || !out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->size == 0) return;
    if (!ix->gp_labels) {  // never labelled: nothing to read
      std::fill(out, out + ix->size, -1);
      return;
    }
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    HIP_CHECK(copy_d2h(out, ix->gp_labels, (size_t)ix->size * 4));
    for (int64_t i = 0; i < ix->size; ++i)
      if (out[i] < 0) out[i] = -1;  // 0x80000000 | slot
  });
}

int clipgpu_index_search_grouped(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                                 float logit_bias, const uint32_t* allow, int64_t* out_idx, float* out_score,
                                 int64_t* out_group) {
  return grouped_host(ix, {queries, nq, k, logit_scale, logit_bias, TOPK_PROBS_NONE, allow}, {out_idx, out_score, out_group});
}

int clipgpu_index_search_grouped_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                        float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t* d_idx,
                                        float* d_score, int64_t* d_group, void* stream) {
  return grouped_device(ix, {d_queries, nq, k, logit_scale, logit_bias, TOPK_PROBS_NONE, d_allow}, {d_idx, d_score, d_group},
                        (hipStream_t)stream);
}

int clipgpu_test_grouped_collapse(int mode) {
  return guarded([&]() {
    if (mode < 0 || mode > 2) throw ClipErr(CLIPGPU_ERR_INVALID, "mode must be 0 (default), 1 (collapse on) or 2 (collapse off)");
    g_grouped_collapse.store(mode);
  });
}

int clipgpu_index_search_compound(clipgpu_index* ix, const float* terms, int64_t n_terms, const int64_t* lims,
                                  int64_t nq, int64_t k, int op, float logit_scale, float logit_bias,
                                  const uint32_t* allow, int64_t* out_idx, float* out_score) {
  return compound_host(ix, {terms, n_terms, nq, k, op, logit_scale, logit_bias, allow}, lims, out_idx, out_score);
}

int clipgpu_index_search_compound_device(clipgpu_index* ix, const float* d_terms, int64_t n_terms, const int32_t* d_lims,
                                         int64_t nq, int64_t max_terms, int64_t k, int op, float logit_scale,
                                         float logit_bias, const uint32_t* d_allow, int64_t* d_idx, float* d_score,
                                         void* stream) {
  return compound_device(ix, {d_terms, n_terms, nq, k, op, logit_scale, logit_bias, d_allow}, d_lims, max_terms, d_idx,
                         d_score, (hipStream_t)stream);
}

int clipgpu_index_search_deep(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                              float logit_bias, const uint32_t* allow, int64_t* out_idx, float* out_score,
                              int32_t* out_passes) {
  return deep_host(ix, {queries, nq, k, logit_scale, logit_bias, allow}, {out_idx, out_score, out_passes});
}

int clipgpu_index_search_deep_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                     float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t* d_idx,
                                     float* d_score, int32_t* d_passes, void* stream) {
  return deep_device(ix, {d_queries, nq, k, logit_scale, logit_bias, d_allow}, {d_idx, d_score, d_passes},
                     (hipStream_t)stream);
}

int clipgpu_index_partition(clipgpu_index* ix, const float* centroids, int64_t C, int64_t* out_counts) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_cluster(ix, !centroids, C);
    HIP_CHECK(hipEventSynchronize(ix->done));  // the filter area, the cluster buffers and the scratch are free
    drop_partition(ix);                        // a failure below leaves the index without a partition, usable
    const ClusterBuf b = cluster_buffers(ix, C, false);
    grow(ix->pt_ids, ix->pt_ids_n, ix->size, (size_t)ix->size * 4);
    grow(ix->pt_off, ix->pt_off_n, C, (size_t)(C + 1) * 4);
    grow(ix->pt_cen, ix->pt_cen_n, C, (size_t)C * ix->E * 4);
    if (!ix->pt_coarse) HIP_CHECK(hipMalloc((void**)&ix->pt_coarse, kCoarseEntries * 20));
    void* tmp = scratch_bytes(ix, lists_tmp_bytes(ix->size));
    hipStream_t s = ix->stream;
    HIP_CHECK(copy_h2d(ix->pt_cen, centroids, (size_t)C * ix->E * 4));
    // the labels of clipgpu_index_assign(centroids, 1, 0, NULL): -1 marks a dead row, which is in no list
    assign_on(ix, (const float*)ix->pt_cen, C, 1.f, 0.f, build_mask(ix, nullptr, s), b.label[0], b.score, s);
    HIP_CHECK(launch_lists(b.label[0], (int)ix->size, (int)C, (int32_t*)ix->pt_off, (int32_t*)ix->pt_ids, tmp, s));
    mark_last(ix, s);
    HIP_CHECK(hipStreamSynchronize(s));
    std::vector<int32_t> off((size_t)C + 1);
    HIP_CHECK(copy_d2h(off.data(), ix->pt_off, off.size() * 4));
    int64_t longest = 0;
    for (int64_t c = 0; c < C; ++c) {
      const int64_t n = (int64_t)off[c + 1] - off[c];
      longest = std::max(longest, n);
      if (out_counts) out_counts[c] = n;
    }
    ix->pt_h_off.swap(off);
    ix->pt_longest = longest;
    ix->pt_C = C;
  });
}

int64_t clipgpu_index_partition_lists(const clipgpu_index* ix) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lk(const_cast<clipgpu_index*>(ix)->mu);
  return ix->pt_C == 0 ? 0 : ix->pt_stale ? -1 : ix->pt_C;
}

int clipgpu_index_get_lists(clipgpu_index* ix, int64_t* out_offsets, int64_t* out_ids) {
  return guarded([&]() {
    if (!ix || !out_offsets || !out_ids) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->pt_C == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "the index has no partition (clipgpu_index_partition)");
    if (ix->pt_stale) throw ClipErr(CLIPGPU_ERR_INVALID, "the partition is stale (call clipgpu_index_partition again)");
    for (size_t c = 0; c < ix->pt_h_off.size(); ++c) out_offsets[c] = ix->pt_h_off[c];
    std::vector<int32_t> ids((size_t)ix->pt_h_off.back());
    if (ids.empty()) return;
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    HIP_CHECK(copy_d2h(ids.data(), ix->pt_ids, ids.size() * 4));
    for (size_t i = 0; i < ids.size(); ++i) out_ids[i] = ids[i];
  });
}

int clipgpu_index_drop_partition(clipgpu_index* ix) {
  return guarded([&]() {
    if (!ix) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    drop_partition(ix);  // the buffers stay for the next partition; destroy frees them
  });
}

int clipgpu_index_search_probed(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, int64_t nprobe,
                                float logit_scale, float logit_bias, const uint32_t* allow, int64_t* out_idx,
                                float* out_score, int64_t* out_probes) {
  return probed_host(ix, {queries, nq, k, nprobe, logit_scale, logit_bias, allow}, {out_idx, out_score, out_probes});
}

int clipgpu_index_search_probed_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k, int64_t nprobe,
                                       float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t* d_idx,
                                       float* d_score, int64_t* d_probes, void* stream) {
  return probed_device(ix, {d_queries, nq, k, nprobe, logit_scale, logit_bias, d_allow}, {d_idx, d_score, d_probes},
                       (hipStream_t)stream);
}

int clipgpu_test_probe_parts(int parts) {
  return guarded([&]() {
    if (parts < 0) throw ClipErr(CLIPGPU_ERR_INVALID, "parts must be >= 0 (0 = default)");
    g_probe_parts.store(parts);
  });
}

int clipgpu_test_probe_chunk(int rows) {
  return guarded([&]() {
    if (rows < 0) throw ClipErr(CLIPGPU_ERR_INVALID, "rows must be >= 0 (0 = default)");
    g_probe_chunk.store(rows);
  });
}

int clipgpu_index_enable_codes(clipgpu_index* ix) {
  return guarded([&]() {
    if (!ix) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->E > kCodesMaxE)
      throw ClipErr(CLIPGPU_ERR_INVALID, "codes need an embedding dim of at most " + std::to_string(kCodesMaxE) +
                                             " (the int32 dot product of two code rows must be exact as an f32), got " +
                                             std::to_string(ix->E));
    if (ix->cd_codes) return;  // enabled already: the codes are current
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    ix->cd_Ep = (ix->E + 63) / 64 * 64;
    hipError_t err = hipMalloc((void**)&ix->cd_codes, (size_t)ix->capacity * ix->cd_Ep);
    if (err == hipSuccess) err = hipMalloc((void**)&ix->cd_scale, (size_t)ix->capacity * 4);
    if (err == hipSuccess) err = hipMalloc((void**)&ix->cd_work, carve_codes(ix, nullptr));
    if (err != hipSuccess) {  // the index stays usable, without codes
      free_codes(ix);
      HIP_CHECK(err);
    }
    code_rows(ix, nullptr, 0, ix->size, ix->stream);
    mark_last(ix, ix->stream);
  });
}

int clipgpu_index_has_codes(const clipgpu_index* ix) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lk(const_cast<clipgpu_index*>(ix)->mu);
  return ix->cd_codes ? 1 : 0;
}

int clipgpu_index_drop_codes(clipgpu_index* ix) {
  return guarded([&]() {
    if (!ix) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->cd_codes) return;
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));  // no search is reading them
    free_codes(ix);
  });
}

int clipgpu_index_get_codes(clipgpu_index* ix, int64_t first, int64_t n, int8_t* out_codes, float* out_scales) {
  return guarded([&]() {
    if (!ix || !out_codes || !out_scales) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->cd_codes) throw ClipErr(CLIPGPU_ERR_INVALID, "the index has no codes (clipgpu_index_enable_codes)");
    check_row_range(ix, first, n);
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    HIP_CHECK(copy_d2h(out_scales, ix->cd_scale + first, (size_t)n * 4));
    // rows of cd_Ep bytes on the device, of E bytes for the caller: in pieces of at most 64 MiB
    const int64_t piece = std::min(n, std::max<int64_t>(1, (64LL << 20) / ix->cd_Ep));
    std::vector<int8_t> h((size_t)piece * ix->cd_Ep);
    for (int64_t r0 = 0; r0 < n; r0 += piece) {
      const int64_t m = std::min(piece, n - r0);
      HIP_CHECK(copy_d2h(h.data(), ix->cd_codes + (first + r0) * ix->cd_Ep, (size_t)m * ix->cd_Ep));
      for (int64_t i = 0; i < m; ++i) memcpy(out_codes + (r0 + i) * ix->E, h.data() + i * ix->cd_Ep, (size_t)ix->E);
    }
  });
}

int clipgpu_index_search_coded(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, int64_t refine,
                               float logit_scale, float logit_bias, const uint32_t* allow, int64_t* out_idx,
                               float* out_score, int64_t* out_cand, float* out_coarse) {
  return coded_host(ix, {queries, nq, k, refine, logit_scale, logit_bias, allow}, {out_idx, out_score, out_cand, out_coarse});
}

int clipgpu_index_search_coded_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k, int64_t refine,
                                      float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t* d_idx,
                                      float* d_score, int64_t* d_cand, float* d_coarse, void* stream) {
  return coded_device(ix, {d_queries, nq, k, refine, logit_scale, logit_bias, d_allow}, {d_idx, d_score, d_cand, d_coarse},
                      (hipStream_t)stream);
}

int clipgpu_test_codes_stage(int stage) {
  return guarded([&]() {
    if (stage < 0 || stage > 2) throw ClipErr(CLIPGPU_ERR_INVALID, "stage must be 0 (both), 1 (coarse) or 2 (re-rank)");
    g_codes_stage.store(stage);
  });
}

int clipgpu_index_range_search_device(clipgpu_index* ix, const float* d_queries, int64_t nq, float threshold,
                                      float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t capacity,
                                      int32_t* d_out_query, int32_t* d_out_row, float* d_out_score,
                                      uint64_t* d_out_total, void* stream) {
  return guarded([&]() {
    const RangeReq r = {threshold, logit_scale, logit_bias, capacity};
    const bool null_arg = !d_queries || !d_out_query || !d_out_row || !d_out_score || !d_out_total;
    const std::unique_lock<std::mutex> lk = enter_range(ix, null_arg, nq, r, "capacity");
    if ((uintptr_t)d_out_total & 7) throw ClipErr(CLIPGPU_ERR_INVALID, "d_out_total must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    order_after_last(ix, s);
    HIP_CHECK(hipMemsetAsync(d_out_total, 0, 8, s));
    const uint32_t* mask = build_mask(ix, d_allow, s);
    const RangeBuf o = {d_out_query, d_out_row, d_out_score, (unsigned long long*)d_out_total};
    for (int64_t q0 = 0; q0 < nq; q0 += kQueryChunk)
      range_chunk(ix, d_queries + q0 * ix->E, (int)std::min(kQueryChunk, nq - q0), q0, false, r, mask, o, s);
    mark_last(ix, s);
  });
}

int clipgpu_index_range_search(clipgpu_index* ix, const float* queries, int64_t nq, float threshold, float logit_scale,
                               float logit_bias, const uint32_t* allow, int64_t max_results, int64_t* out_lims,
                               int64_t* out_idx, float* out_score, int64_t* out_total) {
  return guarded([&]() {
    const RangeReq r = {threshold, logit_scale, logit_bias, max_results};
    const bool null_arg = !queries || !out_lims || !out_idx || !out_score || !out_total;
    const std::unique_lock<std::mutex> lk = enter_range(ix, null_arg, nq, r, "max_results");
    HIP_CHECK(hipEventSynchronize(ix->done));  // the staging buffers, the filter area and the records are free
    const RangeBuf b = result_buffer(ix, max_results);
    if (allow) HIP_CHECK(copy_h2d(ix->d_eff, allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, allow ? ix->d_eff : nullptr, ix->stream);
    HIP_CHECK(hipMemsetAsync(b.total, 0, 8, ix->stream));
    for (int64_t q0 = 0; q0 < nq; q0 += kQueryChunk) {
      const int rows = (int)std::min(kQueryChunk, nq - q0);
      HIP_CHECK(copy_h2d(ix->st_q, queries + q0 * ix->E, (size_t)rows * ix->E * 4));
      range_chunk(ix, ix->st_q, rows, q0, false, r, mask, b, ix->stream);
      HIP_CHECK(hipStreamSynchronize(ix->stream));  // the staged chunk is free again
    }
    mark_last(ix, ix->stream);
    // per query: the search's order, descending score, ties by ascending row
    const std::vector<RangeRec> rec =
        fetch_records(ix, b, max_results, "max_results", out_total, [](const RangeRec& a, const RangeRec& c) {
          return topk_key(a.bits, a.row) > topk_key(c.bits, c.row);
        });
    size_t at = 0;
    for (int64_t q = 0; q <= nq; ++q) {
      while (at < rec.size() && rec[at].query < q) ++at;
      out_lims[q] = (int64_t)at;
    }
    for (size_t i = 0; i < rec.size(); ++i) {
      out_idx[i] = rec[i].row;
      memcpy(&out_score[i], &rec[i].bits, 4);
    }
  });
}

int clipgpu_index_self_join(clipgpu_index* ix, float threshold, float logit_scale, float logit_bias,
                            const uint32_t* allow, int64_t max_pairs, int64_t* out_i, int64_t* out_j, float* out_score,
                            int64_t* out_total) {
  return guarded([&]() {
    const RangeReq r = {threshold, logit_scale, logit_bias, max_pairs};
    const std::unique_lock<std::mutex> lk = enter_range(ix, !out_i || !out_j || !out_score || !out_total, 1, r, "max_pairs");
    HIP_CHECK(hipEventSynchronize(ix->done));
    const RangeBuf b = result_buffer(ix, max_pairs);
    if (allow) HIP_CHECK(copy_h2d(ix->d_eff, allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, allow ? ix->d_eff : nullptr, ix->stream);
    HIP_CHECK(hipMemsetAsync(b.total, 0, 8, ix->stream));
    // chunks of gallery rows are the queries: an f32 gallery's rows in place, a 16-bit gallery's widened into
    // the staged query chunk (stream order keeps a chunk's widening behind the launch that read the last one)
    for (int64_t i0 = 0; i0 < ix->size; i0 += kQueryChunk) {
      const int rows = (int)std::min(kQueryChunk, ix->size - i0);
      const char* src = ix->gallery + i0 * ix->E * ix->esz;
      if (ix->dtype != CLIPGPU_INDEX_F32) HIP_CHECK(launch_gal_widen(ix->dtype, src, ix->st_q, rows * ix->E, ix->stream));
      range_chunk(ix, ix->dtype == CLIPGPU_INDEX_F32 ? (const float*)src : ix->st_q, rows, i0, true, r, mask, b, ix->stream);
    }
    mark_last(ix, ix->stream);
    const std::vector<RangeRec> rec = fetch_records(ix, b, max_pairs, "max_pairs", out_total,
                                                    [](const RangeRec& a, const RangeRec& c) { return a.row < c.row; });
    for (size_t i = 0; i < rec.size(); ++i) {
      out_i[i] = rec[i].query;
      out_j[i] = rec[i].row;
      memcpy(&out_score[i], &rec[i].bits, 4);
    }
  });
}

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
    hipError_t err = hipMalloc((void**)&ix->gallery, (size_t)capacity * E * ix->esz);
    if (err == hipSuccess) err = hipMalloc((void**)&ix->work, carve_work(ix, nullptr));
    if (err == hipSuccess) err = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&ix->done, hipEventDisableTiming);
    if (err != hipSuccess) {
      clipgpu_index_destroy(ix);
      HIP_CHECK(err);
    }
    carve_work(ix, ix->work);
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
  if (ix->res) (void)hipFree(ix->res);
  if (ix->cl_rows) (void)hipFree(ix->cl_rows);
  if (ix->cl_cen) (void)hipFree(ix->cl_cen);
  if (ix->cl_sum) (void)hipFree(ix->cl_sum);
  if (ix->pt_ids) (void)hipFree(ix->pt_ids);
  if (ix->pt_off) (void)hipFree(ix->pt_off);
  if (ix->pt_cen) (void)hipFree(ix->pt_cen);
  if (ix->pt_coarse) (void)hipFree(ix->pt_coarse);
  if (ix->cd_codes) (void)hipFree(ix->cd_codes);
  if (ix->cd_scale) (void)hipFree(ix->cd_scale);
  if (ix->cd_work) (void)hipFree(ix->cd_work);
  if (ix->dp_work) (void)hipFree(ix->dp_work);
  if (ix->cp_work) (void)hipFree(ix->cp_work);
  if (ix->gp_labels) (void)hipFree(ix->gp_labels);
  if (ix->dv_work) (void)hipFree(ix->dv_work);
  if (ix->kn_work) (void)hipFree(ix->kn_work);
  if (ix->cc_work) (void)hipFree(ix->cc_work);
  if (ix->cf_work) (void)hipFree(ix->cf_work);
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
    if (ix->gp_labels && ix->size > 0) {  // every label back to "ungrouped", behind the last search
      HIP_CHECK(hipSetDevice(ix->device));
      HIP_CHECK(hipEventSynchronize(ix->done));
      HIP_CHECK(launch_group_fill((uint32_t*)ix->gp_labels, 0, (long)ix->size, ix->stream));
      mark_last(ix, ix->stream);
    }
    ix->size = 0;  // a later add overwrites the rows only after the last search (the `done` event)
    ix->pt_stale = true;
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
    check_row_range(ix, first, n);
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
    if (mark_rows(ix, ids, n, false)) upload_live(ix);
    mark_last(ix, ix->stream);
  });
}

int clipgpu_index_set_rows(clipgpu_index* ix, const int64_t* ids, const float* rows, int64_t n) {
  return guarded([&]() {
    check_ids(ix, ids, n);
    if (!rows && n > 0) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    check_ids_in_range(ix, ids, n);
    std::vector<int64_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) throw ClipErr(CLIPGPU_ERR_INVALID, "duplicate id");
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    // f32 rows and, behind them, their ids go through the scratch; the scatter kernel rounds them as add does
    for_each_piece(ix, n, 8, [&](int64_t r0, int64_t m, float* f32, void* d_ids) {
      HIP_CHECK(copy_h2d(f32, rows + r0 * ix->E, (size_t)m * ix->E * 4));
      HIP_CHECK(copy_h2d(d_ids, ids + r0, (size_t)m * 8));
      HIP_CHECK(launch_gal_scatter(ix->dtype, f32, (const int64_t*)d_ids, ix->gallery, m, (int)ix->E, ix->stream));
      code_rows(ix, (const int64_t*)d_ids, 0, m, ix->stream);  // the codes of the rows just written, if enabled
      HIP_CHECK(hipStreamSynchronize(ix->stream));
    });
    if (!ix->h_live.empty() && mark_rows(ix, ids, n, true)) upload_live(ix);  // the rows are live again
    ix->pt_stale = true;
    mark_last(ix, ix->stream);
  });
}

int clipgpu_index_add_device(clipgpu_index* ix, const float* d_rows, int64_t n, void* stream) {
  return guarded([&]() {
    check_add(ix, d_rows, n);
    std::lock_guard<std::mutex> lk(ix->mu);
    char* dst = append_at(ix, n);
    HIP_CHECK(hipSetDevice(ix->device));
    hipStream_t s = (hipStream_t)stream;
    order_after_last(ix, s);
    if (ix->dtype == CLIPGPU_INDEX_F32)
      HIP_CHECK(hipMemcpyAsync(dst, d_rows, (size_t)n * ix->E * 4, hipMemcpyDeviceToDevice, s));
    else
      HIP_CHECK(launch_gal_round(ix->dtype, d_rows, dst, n * ix->E, s));
    code_rows(ix, nullptr, ix->size, n, s);  // the codes of the new rows, if enabled
    mark_last(ix, s);
    ix->size += n;
    ix->pt_stale = true;
  });
}

int clipgpu_index_add(clipgpu_index* ix, const float* rows, int64_t n) {
  return guarded([&]() {
    check_add(ix, rows, n);
    std::lock_guard<std::mutex> lk(ix->mu);
    char* dst = append_at(ix, n);
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    if (ix->dtype == CLIPGPU_INDEX_F32) {
      HIP_CHECK(copy_h2d(dst, rows, (size_t)n * ix->E * 4));
    } else {  // the f32 rows go to device scratch and are rounded there
      for_each_piece(ix, n, 0, [&](int64_t r0, int64_t m, float* f32, void*) {
        HIP_CHECK(copy_h2d(f32, rows + r0 * ix->E, (size_t)m * ix->E * 4));
        HIP_CHECK(launch_gal_round(ix->dtype, f32, dst + r0 * ix->E * ix->esz, m * ix->E, ix->stream));
        HIP_CHECK(hipStreamSynchronize(ix->stream));
      });
    }
    if (ix->cd_codes) {  // the codes of the new rows, behind the synchronous copies above
      code_rows(ix, nullptr, ix->size, n, ix->stream);
      mark_last(ix, ix->stream);
    }
    ix->size += n;
    ix->pt_stale = true;
  });
}

int clipgpu_index_dtype(const clipgpu_index* ix) { return ix ? ix->dtype : -1; }

int clipgpu_index_get_rows(clipgpu_index* ix, int64_t first, int64_t n, float* out_rows) {
  return guarded([&]() {
    if (!ix || !out_rows) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    check_row_range(ix, first, n);
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    const char* src = ix->gallery + first * ix->E * ix->esz;
    if (ix->dtype == CLIPGPU_INDEX_F32) {
      HIP_CHECK(copy_d2h(out_rows, src, (size_t)n * ix->E * 4));
      return;
    }
    for_each_piece(ix, n, 0, [&](int64_t r0, int64_t m, float* f32, void*) {
      HIP_CHECK(launch_gal_widen(ix->dtype, src + r0 * ix->E * ix->esz, f32, m * ix->E, ix->stream));
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(out_rows + r0 * ix->E, f32, (size_t)m * ix->E * 4));
    });
  });
}

// The six searches: with or without a filter, with or without probabilities, host or device buffers.
int clipgpu_index_search_filtered_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                         float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t* d_idx,
                                         float* d_score, void* stream) {
  return search_device(ix, {d_queries, nq, k, logit_scale, logit_bias, TOPK_PROBS_NONE, d_allow},
                       {d_idx, d_score, nullptr, nullptr}, (hipStream_t)stream);
}

int clipgpu_index_search_filtered(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                                  float logit_bias, const uint32_t* allow, int64_t* out_idx, float* out_score) {
  return search_host(ix, {queries, nq, k, logit_scale, logit_bias, TOPK_PROBS_NONE, allow},
                     {out_idx, out_score, nullptr, nullptr});
}

int clipgpu_index_search_probs_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                      float logit_scale, float logit_bias, int activation, const uint32_t* d_allow,
                                      int64_t* d_idx, float* d_score, float* d_prob, float* d_norm, void* stream) {
  return search_device(ix, {d_queries, nq, k, logit_scale, logit_bias, probs_kind(activation), d_allow},
                       {d_idx, d_score, d_prob, d_norm}, (hipStream_t)stream);
}

int clipgpu_index_search_probs(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                               float logit_bias, int activation, const uint32_t* allow, int64_t* out_idx,
                               float* out_score, float* out_prob, float* out_norm) {
  return search_host(ix, {queries, nq, k, logit_scale, logit_bias, probs_kind(activation), allow},
                     {out_idx, out_score, out_prob, out_norm});
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

int clipgpu_index_get_rows_at(clipgpu_index* ix, const int64_t* ids, int64_t n, float* out_rows) {
  return guarded([&]() {
    check_ids(ix, ids, n);
    if (!out_rows && n > 0) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    check_ids_in_range(ix, ids, n);
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    // the ids go to the device behind the f32 rows that the gather kernel widens into the scratch
    for_each_piece(ix, n, 8, [&](int64_t r0, int64_t m, float* f32, void* d_ids) {
      HIP_CHECK(copy_h2d(d_ids, ids + r0, (size_t)m * 8));
      HIP_CHECK(launch_gal_gather(ix->dtype, ix->gallery, (const int64_t*)d_ids, f32, m, (int)ix->E, ix->stream));
      HIP_CHECK(hipStreamSynchronize(ix->stream));
      HIP_CHECK(copy_d2h(out_rows + r0 * ix->E, f32, (size_t)m * ix->E * 4));
    });
  });
}

int clipgpu_index_assign_device(clipgpu_index* ix, const float* d_centroids, int64_t C, float logit_scale,
                                float logit_bias, const uint32_t* d_allow, int32_t* d_label, float* d_score,
                                void* stream) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_cluster(ix, !d_centroids || !d_label || !d_score, C);
    if ((uintptr_t)d_centroids & 15) throw ClipErr(CLIPGPU_ERR_INVALID, "d_centroids must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    order_after_last(ix, s);
    assign_on(ix, d_centroids, C, logit_scale, logit_bias, build_mask(ix, d_allow, s), d_label, d_score, s);
    mark_last(ix, s);
  });
}

int clipgpu_index_assign(clipgpu_index* ix, const float* centroids, int64_t C, float logit_scale, float logit_bias,
                         const uint32_t* allow, int64_t* out_label, float* out_score) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_cluster(ix, !centroids || !out_label || !out_score, C);
    HIP_CHECK(hipEventSynchronize(ix->done));  // the filter area and the cluster buffers are free
    const ClusterBuf b = cluster_buffers(ix, C, false);
    if (allow) HIP_CHECK(copy_h2d(ix->d_eff, allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, allow ? ix->d_eff : nullptr, ix->stream);
    HIP_CHECK(copy_h2d(b.cen, centroids, (size_t)C * ix->E * 4));
    assign_on(ix, b.cen, C, logit_scale, logit_bias, mask, b.label[0], b.score, ix->stream);
    mark_last(ix, ix->stream);
    HIP_CHECK(hipStreamSynchronize(ix->stream));
    fetch_assignment(ix, b.label[0], b.score, out_label, out_score);
  });
}

int clipgpu_index_classify_device(clipgpu_index* ix, const float* d_labels, int64_t C, int64_t k, float logit_scale,
                                  float logit_bias, int activation, const uint32_t* d_allow, int32_t* d_label,
                                  float* d_score, float* d_prob, float* d_norm, void* stream) {
  return guarded([&]() {
    const ClassifyReq r = {d_labels, C, k, logit_scale, logit_bias, probs_kind(activation), d_allow};
    const std::unique_lock<std::mutex> lk = enter_classify(ix, r, !d_label || !d_score || !d_prob);
    if ((uintptr_t)d_labels & 15) throw ClipErr(CLIPGPU_ERR_INVALID, "d_labels must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    order_after_last(ix, s);
    classify_on(ix, r, d_labels, build_mask(ix, d_allow, s), {d_label, d_score, d_prob, d_norm}, s);
    mark_last(ix, s);
  });
}

int clipgpu_index_classify(clipgpu_index* ix, const float* labels, int64_t C, int64_t k, float logit_scale,
                           float logit_bias, int activation, const uint32_t* allow, int64_t* out_label,
                           float* out_score, float* out_prob, float* out_norm) {
  return guarded([&]() {
    const ClassifyReq r = {labels, C, k, logit_scale, logit_bias, probs_kind(activation), allow};
    const std::unique_lock<std::mutex> lk = enter_classify(ix, r, !out_label || !out_score || !out_prob);
    HIP_CHECK(hipEventSynchronize(ix->done));  // the filter area and the buffers are free
    grow(ix->cl_cen, ix->cl_cen_n, C, (size_t)C * ix->E * 4);  // the labels go where assign's centroids go
    ClassifyBuf b = classify_buffers(ix, k);
    const bool norm = out_norm && r.probs == TOPK_PROBS_SOFTMAX;  // sigmoid writes none: out_norm stays as it is
    if (!norm) b.norm = nullptr;
    if (allow) HIP_CHECK(copy_h2d(ix->d_eff, allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, allow ? ix->d_eff : nullptr, ix->stream);
    HIP_CHECK(copy_h2d(ix->cl_cen, labels, (size_t)C * ix->E * 4));
    classify_on(ix, r, (const float*)ix->cl_cen, mask, b, ix->stream);
    mark_last(ix, ix->stream);
    HIP_CHECK(hipStreamSynchronize(ix->stream));
    const size_t n = (size_t)(ix->size * k);
    std::vector<int32_t> l(n);
    HIP_CHECK(copy_d2h(l.data(), b.label, n * 4));
    for (size_t i = 0; i < n; ++i) out_label[i] = l[i];
    HIP_CHECK(copy_d2h(out_score, b.score, n * 4));
    HIP_CHECK(copy_d2h(out_prob, b.prob, n * 4));
    if (norm) HIP_CHECK(copy_d2h(out_norm, b.norm, (size_t)ix->size * 8));
  });
}

int clipgpu_index_kmeans(clipgpu_index* ix, int64_t C, float* centroids, int64_t max_iter, const uint32_t* allow,
                         int64_t* out_label, float* out_score, int64_t* out_count, int64_t* out_moved,
                         int64_t* out_iters) {
  return guarded([&]() {
    const bool null_arg = !centroids || !out_label || !out_score || !out_count || !out_moved || !out_iters;
    if (!ix || null_arg) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    if (max_iter < 1) throw ClipErr(CLIPGPU_ERR_INVALID, "max_iter must be at least 1, got " + std::to_string(max_iter));
    const std::unique_lock<std::mutex> lk = enter_cluster(ix, false, C);  // held for the whole call
    HIP_CHECK(hipEventSynchronize(ix->done));
    const ClusterBuf b = cluster_buffers(ix, C, true);
    hipStream_t s = ix->stream;
    const int N = (int)ix->size, E = (int)ix->E;
    if (allow) HIP_CHECK(copy_h2d(ix->d_eff, allow, (size_t)live_words(ix->size) * 4));
    const uint32_t* mask = build_mask(ix, allow ? ix->d_eff : nullptr, s);
    HIP_CHECK(copy_h2d(b.cen, centroids, (size_t)C * E * 4));
    // the shift: m = the largest |x| of the live allowed rows, n = their number
    ClusterStat st;
    HIP_CHECK(hipMemsetAsync(b.stat, 0, sizeof(ClusterStat), s));
    HIP_CHECK(launch_cluster_stats(ix->gallery, ix->dtype, N, E, mask, b.stat, s));
    mark_last(ix, s);
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(copy_d2h(&st, b.stat, sizeof(st)));
    if (st.bad_row)
      throw ClipErr(CLIPGPU_ERR_INVALID, "row " + std::to_string(~st.bad_row) +
                                             " has a non-finite element (k-means sums need finite rows)");
    float m;
    memcpy(&m, &st.max_bits, 4);
    int e = 0, bits = 0;
    if (m != 0.f) (void)std::frexp(m, &e);
    for (unsigned n = st.n; n; n >>= 1) ++bits;
    const int shift = 62 - e - bits;
    // generation `cur` receives labels_t; labels_0 differs from every label and from -1
    int cur = 0;
    HIP_CHECK(hipMemsetAsync(b.label[1], 0xFE, (size_t)N * 4, s));
    for (int64_t t = 0; t < max_iter; ++t) out_moved[t] = -1;
    for (int64_t t = 1;; ++t) {
      HIP_CHECK(hipMemsetAsync(&b.stat->moved, 0, 8, s));
      assign_on(ix, b.cen, C, 1.f, 0.f, mask, b.label[cur], b.score, s);
      HIP_CHECK(launch_cluster_moved(b.label[cur], b.label[cur ^ 1], N, &b.stat->moved, s));
      mark_last(ix, s);
      HIP_CHECK(hipStreamSynchronize(s));  // once per iteration
      unsigned long long moved = 0;
      HIP_CHECK(copy_d2h(&moved, &b.stat->moved, 8));
      out_moved[t - 1] = (int64_t)moved;
      *out_iters = t;
      if (moved == 0) break;  // a fixed point: the centroids are not touched
      HIP_CHECK(hipMemsetAsync(b.sum, 0, (size_t)C * E * 8, s));
      HIP_CHECK(launch_cluster_sums(ix->gallery, ix->dtype, b.label[cur], N, E, shift, b.sum, s));
      HIP_CHECK(launch_cluster_finalise(b.sum, (int)C, E, b.cen, s));
      ix->km_C = C;
      ix->km_shift = shift;
      cur ^= 1;
      if (t == max_iter) {  // unconverged: the labels and scores returned are those of the centroids returned
        assign_on(ix, b.cen, C, 1.f, 0.f, mask, b.label[cur], b.score, s);
        mark_last(ix, s);
        HIP_CHECK(hipStreamSynchronize(s));
        break;
      }
    }
    fetch_assignment(ix, b.label[cur], b.score, out_label, out_score);
    HIP_CHECK(copy_d2h(centroids, b.cen, (size_t)C * E * 4));
    for (int64_t c = 0; c < C; ++c) out_count[c] = 0;
    for (int64_t j = 0; j < ix->size; ++j)
      if (out_label[j] >= 0) ++out_count[out_label[j]];
  });
}

int clipgpu_test_index_kmeans_update(clipgpu_index* ix, const int32_t* d_label, int64_t C, int shift,
                                     float* d_centroids, void* stream) {
  return guarded([&]() {
    const std::unique_lock<std::mutex> lk = enter_cluster(ix, !d_label || !d_centroids, C);
    HIP_CHECK(hipEventSynchronize(ix->done));
    const ClusterBuf b = cluster_buffers(ix, C, true);
    hipStream_t s = (hipStream_t)stream;
    HIP_CHECK(hipMemsetAsync(b.sum, 0, (size_t)C * ix->E * 8, s));
    HIP_CHECK(launch_cluster_sums(ix->gallery, ix->dtype, d_label, (int)ix->size, (int)ix->E, shift, b.sum, s));
    HIP_CHECK(launch_cluster_finalise(b.sum, (int)C, (int)ix->E, d_centroids, s));
    ix->km_C = C;
    ix->km_shift = shift;
    mark_last(ix, s);
  });
}

int clipgpu_test_index_kmeans_sums(clipgpu_index* ix, int64_t C, int64_t* out_sums, int* out_shift) {
  return guarded([&]() {
    if (!ix || !out_sums || !out_shift) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->km_C == 0 || C != ix->km_C) throw ClipErr(CLIPGPU_ERR_INVALID, "no k-means update with this many centroids has run");
    HIP_CHECK(hipSetDevice(ix->device));
    HIP_CHECK(hipEventSynchronize(ix->done));
    HIP_CHECK(copy_d2h(out_sums, ix->cl_sum, (size_t)C * ix->E * 8));
    *out_shift = ix->km_shift;
  });
}

}  // extern "C"

