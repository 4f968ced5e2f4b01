// Compound-query phase 1 of the embedding index (clipgpu_index_search_compound): a query is a group of 1 .. 16
// term vectors, and a gallery row's score is the smallest (all-of, COMPOUND_MIN) or the largest (any-of,
// COMPOUND_MAX) of its term logits.  min and max are not linear, so the group cannot be folded into one query
// vector; here the terms of a group are ROWS OF THE MFMA TILE, and the tile is reduced across its rows before
// anything is selected.  The [terms][N] matrix never exists.
//
//   l_t(j)   = fmaf(dot(term_t, g[j]), scale, bias)             similarity's bits: the same chain, the same k order
//   fused(j) = the l_t(j) whose topk_mono is smallest / largest over the group's terms
//   result   = the k largest topk_key(unmono(fused), j), as bits unmono(fused): a zero is +0.0, a NaN 0x7fc00000
//
// Tile.  The host picks a slot width G in {1, 2, 4, 8, 16}, the smallest that holds the launch's largest group.
// A 16-row query tile holds 16 / G compound queries, query s of the tile in rows [s G, (s + 1) G); a shorter
// group repeats its own first term in the rows it does not fill (compound_gather_kernel lays the rows out once
// per launch).  min and max are idempotent and the rows of an MFMA tile are independent, so the padding needs no
// mask and cannot change a bit.
//
// Block: ONE wave, a 16-row query tile x a gallery span walked in 16-column tiles -- the few-query kernel's
// shape (kernels/topk.hip): the v_mfma_f32_16x16x4_f32 chain through the [k slot][k step] staging of
// topk_stage.hpp in the same k order, slabs of 64 k requested two ahead in one flat sequence over (tile, slab),
// every request the same loads.  After the chain lane (r, qd) holds C[4 qd + e][col r], e < 4.
//
// Fusing.  Each logit becomes its topk_mono u32 once; from there on the reduction is an integer max (for
// COMPOUND_MIN every word is complemented before and after: one kernel argument, no second instantiation):
//   in the lane    G = 2: the pairs (e 0, 1) and (e 2, 3); G >= 4: all four
//   across qd      G >= 8: one exchange with lane ^ 16; G = 16: a second with lane ^ 32
// The exchanges are gfx950's v_permlane16_swap_b32 / v_permlane32_swap_b32 on (x, x): one VALU instruction
// leaves x in one register and x[lane ^ 16] (or ^ 32) in the other, then one v_max_u32.  The alternative,
// ds_bpermute_b32, is an address computation, a trip through the LDS pipe and an lgkmcnt wait in a loop whose
// LDS pipe already carries the staging; the DPP row operations do not cross 16-lane rows.  (Chosen from the
// instruction sequences; the two were not timed against each other.)
//
// Selection.  The tile then carries 16 / G selection rows.  A lane holds 4 (G = 1), 2 (G = 2) or 1 of them; for
// G = 8 the lane groups qd = 1, 3 hold copies and stay out, for G = 16 all but qd = 0.  The key is
// mono << 32 | ~col = topk_key(unmono(fused), col), and the threshold / ballot / append / compact_row selection
// of the few-query kernel runs on 16 / G rows of KC + CAND1 entries.
//
// LDS per block: 11,264 bytes of staging + (16 / G) (KC + 32) 8 bytes of selection state + 64 of counters.
// One wave per block, so the resident waves per CU are min(32 blocks, 160 KiB / LDS):
//
//     KC \ G      1         2         4        8        16
//      16      17,472 9  14,400 11
//      32      19,520 8  15,424 10  13,376 12  12,352 13  11,840 13
//      64      23,616 6  17,472  9
//     128      31,808 5  21,568  7  16,448  9  13,888 11  12,608 12      bytes, waves per CU
//
// (the few-query kernel: the G = 1 column).  From G = 4 on the state is so small that KC 16 and 64 would not add
// a wave over 32 and 128: they are not instantiated.  Registers as compiled: 108 .. 124 VGPRs + 8 AGPRs over a
// 16-bit gallery (4 waves per SIMD at G >= 8, KC 32: the LDS figure stands), 124 .. 140 + 8 over an f32 gallery
// (3 waves per SIMD = 12 per CU, which caps the two cells that say 13).  No instantiation spills.
//
// Grid (query tiles, spans), the query tile fastest: the blocks of one span run together and share its rows in
// cache.  Each block writes its queries' k best to ws[(q * n_spans + span) * k ..], the layout of
// launch_topk_merge, which produces the result.  MASKED as in the few-query kernel: the word of a tile rides
// with the tile's requests; a span with no allowed row writes k empty entries per query and leaves.
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "gallery.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_select.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

// max(v, v[lane ^ 16]) and max(v, v[lane ^ 32]).  The swap of (x, x) leaves the 16-lane rows {0, 0, 2, 2} in
// one operand and {1, 1, 3, 3} in the other (common.hpp explains the asm and its s_nop).
__device__ __forceinline__ uint32_t xmax16_u32(uint32_t v) {
  uint32_t a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return max(a, b);
}
__device__ __forceinline__ uint32_t xmax32_u32(uint32_t v) {
  uint32_t a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return max(a, b);
}

// The inverse of topk_mono on its image: the canonical bits of a fused score.
__device__ __forceinline__ uint32_t unmono(uint32_t m) {
  if (m == 0u) return kTopkEmptyScore;  // NaN
  return (m & 0x80000000u) ? (m & 0x7fffffffu) : ~m;
}

// The padded tile rows of one launch.  Row 16 t + s of out holds term j = s % G of query q = t * (16 / G) + s / G
// (queries past nq - 1: the last one; they are never selected), or the query's first term where j is past its
// group.  lims: the launch's nq + 1 offsets into terms; a group is clamped to 1 .. G terms and a term to
// [0, T), so that offsets that are not what the caller promised read other terms, never other memory.
__global__ __launch_bounds__(256) void compound_gather_kernel(const float* __restrict__ terms, long T,
                                                              const int32_t* __restrict__ lims, int nq, int G, int E,
                                                              float* __restrict__ out, long rows) {
  const int per = E / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rows * per; i += (long)gridDim.x * 256) {
    const long row = i / per;
    const int s = (int)(row & 15);
    const int q = min((int)((row >> 4) * (16 / G)) + s / G, nq - 1), j = s % G;
    const long first = lims[q];
    const long n = min(max((long)lims[q + 1] - first, 1L), (long)G);
    const long t = min(max(first + (j < n ? j : 0), 0L), T - 1);
    ((float4*)out)[i] = ((const float4*)terms)[t * per + (i - row * per)];
  }
}

// KC: list capacity the LDS is sized for (k <= KC).  G: the slot width.  flip: ~0 for COMPOUND_MIN, 0 for MAX.
template <int KC, typename GT, bool MASKED, int G>
__global__ __launch_bounds__(64) void topk_compound_kernel(const float* __restrict__ tq, const GT* __restrict__ gal,
                                                           int nq, int N, int E, float scale, float bias, int k,
                                                           uint32_t flip, int span_cols, int n_spans,
                                                           uint2* __restrict__ ws, const uint32_t* __restrict__ mask) {
  typedef typename GalRaw<GT>::type raw_t;
  constexpr int STRIDE = KC + CAND1;
  constexpr int NR = NB / G;                         // selection rows = compound queries of the tile
  constexpr int RPL = G == 1 ? 4 : G == 2 ? 2 : 1;   // selection rows a lane holds
  __shared__ __attribute__((aligned(16))) float stage[2][NB * LDT];  // A | B: [row][k slot qd][k step]
  __shared__ uint2 sel[NR * STRIDE];
  __shared__ int cnt[NB];
  const int lane = threadIdx.x, tile = blockIdx.x, span = blockIdx.y;
  const int q0 = tile * NR;  // the tile's first compound query; q0 < nq
  const unsigned c_begin = (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {  // a span with no allowed row: k empty entries per query, nothing requested
    unsigned any = 0;
    for (unsigned w = (c_begin >> 5) + lane; w < ((c_end + 63) >> 6) * 2; w += 64) any |= mask[w];
    if (__ballot(any != 0) == 0) {
      for (int row = 0; row < NR && q0 + row < nq; ++row) {
        uint2* dst = ws + ((long)(q0 + row) * n_spans + span) * k;
        for (int t = lane; t < k; t += 64) dst[t] = ent_empty();
      }
      return;
    }
  }
  for (int i = lane; i < NR * STRIDE; i += 64) sel[i] = ent_empty();
  if (lane < NB) cnt[lane] = 0;
  wave_lds_order();
  const int r = lane & 15, qd = lane >> 4;
  // the selection row of lane group g for the lane's e-th value, and whether the group selects at all
  auto row_of = [](int g, int e) { return G <= 4 ? g * RPL + e : G == 8 ? g >> 1 : 0; };
  const bool owner = G <= 4 ? true : G == 8 ? (qd & 1) == 0 : qd == 0;
  uint64_t thr[RPL];  // thresholds of rows row_of(qd, e)
#pragma unroll
  for (int e = 0; e < RPL; ++e) thr[e] = 0;
  // Staging as in the few-query kernel: lane -> (rows lane / 16 + 4 p, p < 4; k step lane % 16).  Every row of
  // the tile exists (the gather pads), so the query side needs no clamp.
  const int srow = lane >> 4, sj = lane & 15;
  const float* pa[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pa[p] = tq + ((long)tile * NB + p * 4 + srow) * E;
  unsigned lj = c_begin;  // the next slab to request: tile lj, k lk
  int lk = 0;
  // Every request is the same eight loads (and the tile's mask word, MASKED) whatever the position, so that
  // the compiler can count the loads in flight; topk.hip (request) has the reasons and the clamps.
  auto request = [&](float4(&va)[4], raw_t(&vb)[4], uint32_t& vm) {
    const int ko = min(lk + sj * 4, E - 4);
    if constexpr (MASKED) vm = mask[min(lj + 4 * srow, (unsigned)N - 1) >> 5];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      va[p] = *(const float4*)(pa[p] + ko);
      vb[p] = gal_raw(gal + (long)min(lj + p * 4 + srow, (unsigned)N - 1) * E + ko);
    }
    lk += TK;
    if (lk >= E) {
      lk = 0;
      lj += NB;
    }
  };
  auto put = [&](float* dst, int p, float4 v) {
    float* d = dst + (p * 4 + srow) * LDT + sj;
    d[0] = v.x; d[KQ] = v.y; d[2 * KQ] = v.z; d[3 * KQ] = v.w;
  };
  // C[row = 4 * qd + e][col = r] of the tile at column cj: fuse the rows of each slot, then the few-query
  // kernel's selection on the NR fused rows.
  auto select = [&](unsigned cj, const f32x4& acc, bool allowed) {
    uint32_t m[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = topk_mono(__float_as_uint(fmaf(acc[e], scale, bias))) ^ flip;
    uint32_t v[RPL];
    if constexpr (G == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = m[e];
    } else if constexpr (G == 2) {
      v[0] = max(m[0], m[1]);
      v[1] = max(m[2], m[3]);
    } else {
      v[0] = max(max(m[0], m[1]), max(m[2], m[3]));
      if constexpr (G >= 8) v[0] = xmax16_u32(v[0]);
      if constexpr (G == 16) v[0] = xmax32_u32(v[0]);
    }
    const unsigned col = cj + r;
#pragma unroll
    for (int e = 0; e < RPL; ++e) {
      const int rl = row_of(qd, e);
      const uint32_t mono = v[e] ^ flip;
      const uint64_t key = ((uint64_t)mono << 32) | (uint32_t)~col;  // topk_key(unmono(mono), col)
      const bool live = owner && col < c_end && q0 + rl < nq && allowed;
      bool pass = live && key > thr[e];
      uint64_t bal = __ballot(pass);
      if (bal == 0) continue;  // wave-uniform: the common case once the thresholds have warmed up
      unsigned mq = (unsigned)(bal >> (16 * qd)) & 0xffffu;
      int c = cnt[rl];
      if (__ballot(c + __popc(mq) > CAND1) != 0) {
        for (int g = 0; g < 4; ++g) {  // the rows this ballot covers (a group that is no owner has no bit in it)
          const int row = row_of(g, e);
          const int c2 = cnt[row];
          if (c2 + __popc((unsigned)(bal >> (16 * g)) & 0xffffu) > CAND1) {
            const uint64_t t2 = compact_row(sel + row * STRIDE, k, c2, lane);
            if (lane == 0) cnt[row] = 0;
            if (qd == g) thr[e] = t2;
            wave_lds_order();
          }
        }
        wave_lds_order();
        pass = live && key > thr[e];
        bal = __ballot(pass);
        mq = (unsigned)(bal >> (16 * qd)) & 0xffffu;
        c = cnt[rl];
      }
      if (pass) sel[rl * STRIDE + k + c + __popc(mq & ((1u << r) - 1u))] = make_uint2(unmono(mono), col);
      wave_lds_order();
      if (r == 0 && mq != 0) cnt[rl] = c + __popc(mq);
      wave_lds_order();
    }
  };
  unsigned cj = c_begin;  // the slab in hand: tile cj, k ck
  int ck = 0;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step = [&](float4(&va)[4], raw_t(&vb)[4], uint32_t& vm) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      put(stage[0], p, va[p]);
      put(stage[1], p, gal_widen<GT>(vb[p]));
    }
    // the bit of column cj + r, taken before the request below reuses the word's register (topk.hip, step)
    uint32_t mbit = 1;
    if constexpr (MASKED) {
      mbit = (vm >> ((cj & 16) + r)) & 1u;
      asm volatile("" : "+v"(mbit));
    }
    const bool allowed = mbit != 0;
    wave_lds_order();
    request(va, vb, vm);  // two slabs ahead; the slab after this one is already in flight
    const int steps = min(TK, E - ck) / 4;  // a multiple of 4 (E % 16 == 0): the last slab may be short
    // 16x16x4: lane (r, qd) supplies A[r][qd] and B[qd][r]; k = ck + 4 * (4 jq + st) + qd, ascending
    const float* fa = &stage[0][r * LDT + qd * KQ];
    const float* fb = &stage[1][r * LDT + qd * KQ];
    if (steps == TK / 4) {  // a full slab: all eight fragment reads go out before the first MFMA waits
      f32x4 a[4], b[4];
#pragma unroll
      for (int jq = 0; jq < 4; ++jq) {
        a[jq] = *(const f32x4*)(fa + jq * 4);
        b[jq] = *(const f32x4*)(fb + jq * 4);
      }
#pragma unroll
      for (int jq = 0; jq < 4; ++jq)
#pragma unroll
        for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jq][st], b[jq][st], acc, 0, 0, 0);
    } else {
#pragma unroll
      for (int jq = 0; jq < 3; ++jq) {
        if (jq * 4 >= steps) break;
        const f32x4 a = *(const f32x4*)(fa + jq * 4);
        const f32x4 b = *(const f32x4*)(fb + jq * 4);
#pragma unroll
        for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st], b[st], acc, 0, 0, 0);
      }
    }
    wave_lds_order();  // the fragment reads come before the next slab's stores
    ck += TK;
    if (ck >= E) {
      select(cj, acc, allowed);
      acc = f32x4{0.f, 0.f, 0.f, 0.f};
      ck = 0;
      cj += NB;
    }
  };
  float4 a0[4] = {}, a1[4] = {};
  raw_t b0[4] = {}, b1[4] = {};
  uint32_t m0 = 0, m1 = 0;
  // The steps run in pairs, a fixed number of them (topk.hip has the reasons): an odd count ends in one step past
  // the span, which stages clamped rows and, if it completes a tile, selects nothing (every column >= c_end).
  request(a0, b0, m0);
  __builtin_amdgcn_sched_barrier(0);
  request(a1, b1, m1);
  __builtin_amdgcn_sched_barrier(0);
  const int n_steps = (int)((c_end - c_begin + NB - 1) / NB) * ((E + TK - 1) / TK);
  for (int it = 0; it < n_steps; it += 2) {
    step(a0, b0, m0);
    step(a1, b1, m1);
  }
  for (int row = 0; row < NR && q0 + row < nq; ++row) {
    const int c2 = cnt[row];
    if (c2 > 0) compact_row(sel + row * STRIDE, k, c2, lane);
    uint2* dst = ws + ((long)(q0 + row) * n_spans + span) * k;
    for (int t = lane; t < k; t += 64) dst[t] = sel[row * STRIDE + t];
  }
}

template <int KC, typename GT, bool MASKED, int G>
void launch_compound_one(const CompoundArgs& a) {
  const TopkPlan& p = a.plan;
  hipLaunchKernelGGL((topk_compound_kernel<KC, GT, MASKED, G>), dim3((a.nq * G + NB - 1) / NB, p.n_spans), dim3(64), 0,
                     a.stream, a.tiles, (const GT*)a.g, a.nq, a.N, a.E, a.scale, a.bias, a.k,
                     a.op == COMPOUND_MIN ? ~0u : 0u, p.span_cols, p.n_spans, (uint2*)a.ws, a.mask);
}

// Every instantiation: [gallery type][MASKED][slot width 1 / 2 / 4 / 8 / 16][list capacity 16 / 32 / 64 / 128].
// From G = 4 on the capacities 16 and 64 take the next one up (the file header has the LDS table).
typedef void (*Compound)(const CompoundArgs&);
#define COMPOUND_KC4(GT, M, G) \
  { launch_compound_one<16, GT, M, G>, launch_compound_one<32, GT, M, G>, launch_compound_one<64, GT, M, G>, \
    launch_compound_one<128, GT, M, G> }
#define COMPOUND_KC2(GT, M, G) \
  { launch_compound_one<32, GT, M, G>, launch_compound_one<32, GT, M, G>, launch_compound_one<128, GT, M, G>, \
    launch_compound_one<128, GT, M, G> }
#define COMPOUND_M(GT, M) \
  { COMPOUND_KC4(GT, M, 1), COMPOUND_KC4(GT, M, 2), COMPOUND_KC2(GT, M, 4), COMPOUND_KC2(GT, M, 8), COMPOUND_KC2(GT, M, 16) }
#define COMPOUND_GT(GT) \
  { COMPOUND_M(GT, false), COMPOUND_M(GT, true) }
constexpr Compound kCompound[3][2][5][4] = {COMPOUND_GT(float), COMPOUND_GT(_Float16), COMPOUND_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kCompound");

}  // namespace

int compound_width(int largest) { return largest <= 1 ? 1 : largest <= 2 ? 2 : largest <= 4 ? 4 : largest <= 8 ? 8 : 16; }

TopkPlan compound_plan(long N, int nq, int G, int max_blocks) {
  const long tiles = (N + TB - 1) / TB, qtiles = ((long)nq * G + NB - 1) / NB;
  // spans: a one-wave block each, kNarrowSpans blocks fill the GPU; the workspace holds 64 * max_blocks query
  // rows of kTopkMax entries, a launch writes nq * n_spans rows of k
  const long most = std::max(1L, std::min({kNarrowSpans / qtiles, 64L * max_blocks / nq, 65535L}));
  long want = std::min(tiles, most);
  const long forced = g_topk_span_cols.load();
  if (forced > 0) want = std::min(most, (tiles + forced / TB - 1) / (forced / TB));
  TopkPlan p;
  p.narrow = true;
  p.span_cols = (int)((tiles + want - 1) / want) * TB;
  p.n_spans = (int)((N + p.span_cols - 1) / p.span_cols);
  return p;
}

hipError_t launch_compound_gather(const float* terms, long T, const int32_t* lims, int nq, int G, int E, float* tiles,
                                  hipStream_t s) {
  if (!terms || !lims || !tiles || T <= 0 || nq <= 0 || E <= 0 || E % 16 != 0 || compound_width(G) != G)
    return hipErrorInvalidValue;
  if (((uintptr_t)terms | (uintptr_t)tiles) & 15) return hipErrorInvalidValue;
  const long rows = ((long)nq * G + NB - 1) / NB * NB, work = rows * (E / 4);
  hipLaunchKernelGGL(compound_gather_kernel, dim3((int)std::min<long>((work + 255) / 256, 4096)), dim3(256), 0, s, terms,
                     T, lims, nq, G, E, tiles, rows);
  return hipGetLastError();
}

hipError_t launch_compound(const CompoundArgs& a) {
  const TopkPlan& p = a.plan;
  if (!a.tiles || !a.g || !a.ws) return hipErrorInvalidValue;
  if (a.nq <= 0 || a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.k < 1 || a.k > kTopkMax) return hipErrorInvalidValue;
  if (compound_width(a.G) != a.G || (a.op != COMPOUND_MIN && a.op != COMPOUND_MAX)) return hipErrorInvalidValue;
  if (p.span_cols <= 0 || p.span_cols % TB != 0 || (long)p.n_spans * p.span_cols < a.N ||
      (long)(p.n_spans - 1) * p.span_cols >= a.N || (long)p.n_spans * a.k > INT32_MAX || p.n_spans > 65535)
    return hipErrorInvalidValue;
  if (a.mask && ((uintptr_t)a.mask & 7)) return hipErrorInvalidValue;
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  const int kc = a.k <= 16 ? 0 : a.k <= 32 ? 1 : a.k <= 64 ? 2 : 3;
  const int gi = a.G == 1 ? 0 : a.G == 2 ? 1 : a.G == 4 ? 2 : a.G == 8 ? 3 : 4;
  kCompound[a.dtype][a.mask != nullptr][gi][kc](a);
  return hipGetLastError();
}

}  // namespace clipgpu
