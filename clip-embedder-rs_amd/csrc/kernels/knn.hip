// Nearest neighbours of stored rows and the k-NN graph (clipgpu_index_neighbors): per query row i of the
// gallery, the k best gallery rows j != i -- the search's scores, order and workspace, with the query operand
// taken from the gallery itself.
//
//   score[i][j] = fmaf(dot(g[i], g[j]), scale, bias)         the bits of launch_topk for the query widen(g[i])
//   order       = descending score, ties by ascending j       (topk_key.hpp)
//
// Phase 1 (knn_partial_kernel): a block is one panel of 64 query rows x one gallery span, 4 waves x 16 rows
// as in topk.hip's wide kernel, so a row's selection state belongs to one wave.  Row r of panel p is gallery
// row ids[p * 64 + r], or id0 + p * 64 + r without ids (the graph).  What differs from the wide kernel:
//   * The A operand is loaded from the gallery in its own element type (gal_raw), kept as loaded while the
//     loads are in flight and widened when it is staged, like the column operand, through the same
//     [k slot][k step] layout: one MFMA chain (v_mfma_f32_16x16x4_f32, k ascending) with the search's bits.
//     There is no f32 copy of the queries and no gather pass; a 16-bit gallery is read as 16 bits twice.
//   * A column equal to the row's own id never passes the ballot.  Without ids only the tiles that overlap
//     the panel's own 64 rows can hold one: a block-uniform test picks the selection with the comparison for
//     those and the plain one for every other tile.  With ids every tile compares, one v_cmp per lane and
//     16-column tile.
//   * A query row is invalid when it lies past nq, its id is outside [0, N) or its bit in qvalid is clear.
//     Its threshold starts at the largest key, so nothing ever passes and its entries stay empty; its loads
//     are clamped to row 0.  A panel with no valid row, like a span with no allowed column, writes empty
//     entries and leaves before it stages anything.
//   * The grid is one-dimensional, panel fastest: the blocks dispatched together are the panels of one span,
//     walking it from its first tile, so concurrent panels read the same gallery tiles.
// Phase 2 is launch_topk_merge, unchanged.  The selection (thresholds, ballot, compact_row), the mask words and
// the 64-k slab staging are topk_select.hpp / topk_stage.hpp / topk_key.hpp; the ballot / compact / append
// block is written out here as it is in topk.hip's two kernels (see the note there on sharing it).
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "gallery.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_select.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

constexpr int kKnnWideFrom = 512;  // panels from which a call is cut into one span (two blocks per CU at KC <= 32)

// KC: list capacity the LDS is sized for (k <= KC), blocks per CU as in the wide search kernel.
template <int KC, typename GT, bool MASKED>
__global__ __launch_bounds__(256, KC <= 32 ? 2 : 1) void knn_partial_kernel(
    const GT* __restrict__ gal, const int64_t* __restrict__ ids, long id0, int nq, int N, int E, float scale, float bias,
    int k, int span_cols, int n_spans, int n_panels, uint2* __restrict__ ws, const uint2* __restrict__ mask,
    const uint32_t* __restrict__ qvalid) {
  typedef typename GalRaw<GT>::type raw_t;
  constexpr int STRIDE = KC + CAND1;
  __shared__ __attribute__((aligned(16))) float stage[2][TB * LDT];  // A | B: [row][k slot qd][k step]
  __shared__ uint2 sel[TB * STRIDE];
  __shared__ int cnt[TB];
  __shared__ unsigned qrow[TB];   // the gallery row a query row loads: its id, or 0 for an id out of range
  __shared__ unsigned qself[TB];  // a valid query row's id (the column it must not take), else kTopkEmptyIndex
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int panel = blockIdx.x % n_panels, span = blockIdx.x / n_panels;
  const int i0 = panel * TB;
  const unsigned c_begin = (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  bool valid = false;
  if (tid < TB) {
    const int g = i0 + tid;
    const long id = g < nq ? (ids ? (long)ids[g] : id0 + g) : -1;
    const bool in = id >= 0 && id < N;
    valid = in;
    if constexpr (MASKED)
      if (in && qvalid) valid = ((qvalid[id >> 5] >> (id & 31)) & 1u) != 0;
    qrow[tid] = in ? (unsigned)id : 0u;
    qself[tid] = valid ? (unsigned)id : kTopkEmptyIndex;
  }
  bool work = __syncthreads_or((int)valid) != 0;  // also: qrow and qself are written
  if constexpr (MASKED) {
    unsigned any = 0;
    for (unsigned t = (c_begin >> 6) + tid; t < ((c_end + 63) >> 6); t += 256) any |= mask[t].x | mask[t].y;
    work = (__syncthreads_or((int)(any != 0)) != 0) && work;
  }
  if (!work) {  // block-uniform: no valid query row or no allowed column; k empty entries per row, nothing staged
    for (int row = wave * 16; row < wave * 16 + 16; ++row)
      if (i0 + row < nq) {
        uint2* dst = ws + ((long)(i0 + row) * n_spans + span) * k;
        for (int t = lane; t < k; t += 64) dst[t] = ent_empty();
      }
    return;
  }
  for (int i = tid; i < TB * STRIDE; i += 256) sel[i] = ent_empty();
  if (tid < TB) cnt[tid] = 0;
  __syncthreads();
  const int rowbase = wave * 16;
  const int r = lane & 15, qd = lane >> 4;
  uint64_t thr[4];   // thresholds of rows rowbase + 4 * qd + e: the largest key for an invalid row
  unsigned self[4];  // their own ids
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    self[e] = qself[rowbase + 4 * qd + e];
    thr[e] = self[e] == kTopkEmptyIndex ? ~0ull : 0ull;
  }
  // Staging as in the wide search kernel, for both operands: thread -> (rows tid / 16 + 16 p, p < 4; k step
  // tid % 16), one raw_t = the four k slots of one step; the next slab's loads are issued before this slab's
  // MFMAs.
  const int srow = tid >> 4, sj = tid & 15;
  auto loadg = [&](raw_t(&v)[4], const GT* const(&src)[4], int k0) {
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = k0 + sj * 4 < E ? gal_raw(src[p] + k0) : raw_t{};  // zero bits widen to 0.f
  };
  auto put = [&](float* dst, const raw_t(&v)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float4 w = gal_widen<GT>(v[p]);
      float* d = dst + (p * 16 + srow) * LDT + sj;
      d[0] = w.x; d[KQ] = w.y; d[2 * KQ] = w.z; d[3 * KQ] = w.w;
    }
  };
  // C[row = 4 * qd + e][col = r] of column tile t: the wide kernel's selection.  SELF: the tile may hold a
  // row's own column, which then does not pass, before the threshold is looked at.
  auto select = [&](auto self_c, unsigned j0, uint2 mw, const f32x4(&acc)[4]) {
    constexpr bool SELF = decltype(self_c)::value;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned col = j0 + t * 16 + r;
        const uint32_t bits = __float_as_uint(fmaf(acc[t][e], scale, bias));
        const uint64_t key = topk_key(bits, col);
        bool ok = col < c_end;
        if constexpr (MASKED) ok = ok && (((t < 2 ? mw.x : mw.y) >> ((t & 1) * 16 + r)) & 1u) != 0;
        if constexpr (SELF) ok = ok && col != self[e];
        bool pass = ok && key > thr[e];
        uint64_t bal = __ballot(pass);
        if (bal == 0) continue;  // wave-uniform: the common case once the thresholds have warmed up
        const int rl = rowbase + 4 * qd + e;
        unsigned mq = (unsigned)(bal >> (16 * qd)) & 0xffffu;
        int c = cnt[rl];
        if (__ballot(c + __popc(mq) > CAND1) != 0) {
          for (int g = 0; g < 4; ++g) {  // the four rows this ballot covers
            const int row = rowbase + 4 * g + e;
            const int c2 = cnt[row];
            if (c2 + __popc((unsigned)(bal >> (16 * g)) & 0xffffu) > CAND1) {
              const uint64_t t2 = compact_row(sel + row * STRIDE, k, c2, lane);
              if (lane == 0) cnt[row] = 0;
              if (qd == g) thr[e] = t2;
            }
          }
          wave_lds_order();
          pass = ok && key > thr[e];
          bal = __ballot(pass);
          mq = (unsigned)(bal >> (16 * qd)) & 0xffffu;
          c = cnt[rl];
        }
        if (pass) sel[rl * STRIDE + k + c + __popc(mq & ((1u << r) - 1u))] = make_uint2(bits, col);
        wave_lds_order();
        if (r == 0 && mq != 0) cnt[rl] = c + __popc(mq);
        wave_lds_order();
      }
  };
  const GT* pa[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pa[p] = gal + (long)qrow[p * 16 + srow] * E + sj * 4;
  const long own = id0 + i0;  // without ids: the panel's rows are columns own .. own + 63
  for (unsigned j0 = c_begin; j0 < c_end; j0 += TB) {
    uint2 mw = make_uint2(0, 0);  // the tile's allowed bits: columns j0 .. j0 + 31 | j0 + 32 .. j0 + 63
    if constexpr (MASKED) {
      mw = mask[j0 >> 6];
      if ((mw.x | mw.y) == 0) continue;  // block-uniform, before the tile's loads and barriers
    }
    const GT* pb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) pb[p] = gal + (long)min(j0 + p * 16 + srow, (unsigned)N - 1) * E + sj * 4;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    raw_t va[4], vb[4];
    loadg(va, pa, 0);
    loadg(vb, pb, 0);
    for (int k0 = 0; k0 < E; k0 += TK) {
      __syncthreads();
      put(stage[0], va);
      put(stage[1], vb);
      __syncthreads();
      if (k0 + TK < E) {
        loadg(va, pa, k0 + TK);
        loadg(vb, pb, k0 + TK);
      }
      const int steps = min(TK, E - k0) / 4;  // a multiple of 4 (E % 16 == 0): the last slab may be short
#pragma unroll
      for (int jq = 0; jq < 4; ++jq) {
        if (jq * 4 >= steps) break;
        // 16x16x4: lane (r, qd) supplies A[r][qd] and B[qd][r]; k = k0 + 4 * (4 jq + st) + qd, ascending
        const f32x4 a = *(const f32x4*)&stage[0][(rowbase + r) * LDT + qd * KQ + jq * 4];
        f32x4 b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = *(const f32x4*)&stage[1][(t * 16 + r) * LDT + qd * KQ + jq * 4];
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st], b[t][st], acc[t], 0, 0, 0);
      }
    }
    // block-uniform: with ids any tile may hold a row's own column, without them only those over the panel's rows
    if (ids != nullptr || ((long)j0 < own + TB && (long)j0 + TB > own)) select(std::true_type{}, j0, mw, acc);
    else select(std::false_type{}, j0, mw, acc);
  }
  for (int g = 0; g < 16; ++g) {
    const int row = rowbase + g;
    const int c2 = cnt[row];
    if (c2 > 0) compact_row(sel + row * STRIDE, k, c2, lane);
    if (i0 + row < nq) {
      uint2* dst = ws + ((long)(i0 + row) * n_spans + span) * k;
      for (int t = lane; t < k; t += 64) dst[t] = sel[row * STRIDE + t];
    }
  }
}

template <int KC, typename GT, bool MASKED>
void launch_knn_phase1(const KnnArgs& a) {
  const int panels = (a.nq + TB - 1) / TB;
  hipLaunchKernelGGL((knn_partial_kernel<KC, GT, MASKED>), dim3(panels * a.plan.n_spans), dim3(256), 0, a.stream,
                     (const GT*)a.g, a.ids, a.id0, a.nq, a.N, a.E, a.scale, a.bias, a.k, a.plan.span_cols, a.plan.n_spans,
                     panels, (uint2*)a.ws, (const uint2*)a.mask, a.qvalid);
}

// Every instantiation: [gallery type][MASKED][list capacity 16 / 32 / 64 / 128].
typedef void (*KnnPhase1)(const KnnArgs&);
#define KNN_KC(GT, M) \
  { launch_knn_phase1<16, GT, M>, launch_knn_phase1<32, GT, M>, launch_knn_phase1<64, GT, M>, launch_knn_phase1<128, GT, M> }
#define KNN_GT(GT) { KNN_KC(GT, false), KNN_KC(GT, true) }
constexpr KnnPhase1 kKnnPhase1[3][2][4] = {KNN_GT(float), KNN_GT(_Float16), KNN_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kKnnPhase1");

}  // namespace

TopkPlan knn_plan(long N, long panels, int max_blocks) {
  const long tiles = (N + TB - 1) / TB;
  // Few panels: the search's cut, as many spans as the workspace of max_blocks blocks holds for them, so that one
  // id still fills the chip.  From kKnnWideFrom panels on the panels alone do, and one span spares the merge.
  long want = panels >= kKnnWideFrom ? 1 : std::min(tiles, std::max(1L, max_blocks / std::max(1L, panels)));
  const long forced = g_topk_span_cols.load();
  if (forced > 0) want = std::min<long>(max_blocks, (tiles + forced / TB - 1) / (forced / TB));
  TopkPlan p;
  p.narrow = false;
  p.span_cols = (int)((tiles + want - 1) / want) * TB;
  p.n_spans = (int)((N + p.span_cols - 1) / p.span_cols);
  return p;
}

long knn_launch_rows(const TopkPlan& p, int k, int max_blocks) {
  return std::max(1L, (long)max_blocks * kTopkMax / ((long)p.n_spans * k)) * TB;
}

hipError_t launch_knn(const KnnArgs& a) {
  const TopkPlan& p = a.plan;
  if (!a.g || !a.ws || !a.out_idx || !a.out_score) return hipErrorInvalidValue;
  if (a.nq <= 0 || a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.k < 1 || a.k > kTopkMax || a.id0 < 0) return hipErrorInvalidValue;
  if (p.span_cols <= 0 || p.span_cols % TB != 0 || (long)p.n_spans * p.span_cols < a.N ||
      (long)(p.n_spans - 1) * p.span_cols >= a.N || p.n_spans > 65535)
    return hipErrorInvalidValue;
  const long panels = (a.nq + TB - 1) / TB;
  if (panels * TB * p.n_spans * a.k > a.ws_entries || panels * p.n_spans > INT32_MAX) return hipErrorInvalidValue;
  if (a.mask && ((uintptr_t)a.mask & 7)) return hipErrorInvalidValue;
  if (a.qvalid && !a.mask) return hipErrorInvalidValue;  // the unmasked kernels read no validity bits
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  const int kc = a.k <= 16 ? 0 : a.k <= 32 ? 1 : a.k <= 64 ? 2 : 3;
  kKnnPhase1[a.dtype][a.mask != nullptr][kc](a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_topk_merge(a.ws, a.nq, p.n_spans, a.k, a.out_idx, a.out_score, a.stream);
}

}  // namespace clipgpu
