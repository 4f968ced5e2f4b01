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

}  // namespace

extern "C" {

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

