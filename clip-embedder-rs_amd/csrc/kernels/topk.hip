// Fused top-k search of a device-resident gallery (clipgpu_index_search): the k best gallery rows
// per query, without the [n_q][N] score matrix ever existing in memory.
//
//   score[i][j] = fmaf(dot(q[i], g[j]), scale, bias)        bit-identical to sim_logits_kernel
//   order       = descending score, ties by ascending j      (topk_key.hpp)
//
// The dot products are the exact-f32-input MFMA of similarity.hip (v_mfma_f32_16x16x4_f32, k
// ascending: bitwise a fmaf chain, so neither the tiling nor the LDS staging shows in the bits).  Here a wave owns 16 query rows x all 64 columns of a tile (1 x 4 MFMA tiles), so every
// row's selection state belongs to one wave and the selection needs no block barrier.
//
// Phase 1 (topk_partial_kernel): grid (gallery spans x 64-query tiles).  A block walks its span in
// 64-column tiles.  Per query row it keeps, in LDS, the k best (score, index) entries seen so far
// (sorted) and a small candidate buffer; the key of the k-th best is the row's threshold, held in
// registers.  After a tile's MFMAs each lane tests its 16 scores against the thresholds; a wave
// ballot finds the (rare, once the threshold has warmed up) passing lanes, which append themselves
// to their row's candidate buffer at ballot-prefix positions.  A buffer that would overflow is
// compacted first: the k best of (list + candidates), by rank counting -- keys are unique, so an
// entry's rank is its sorted position.  The span's k best per row go to a workspace.
// Phase 2 (topk_merge_kernel): one wave per query row runs the same threshold / ballot / compact
// selection over the row's n_spans * k workspace entries and writes int64 indices and f32 scores,
// best first; slots beyond min(k, N) are (-1, -inf).
//
// The gallery is stored as f32, f16 or bf16 (TopkGal; rounded by kernels/gallery.hip); a 16-bit element is widened
// in registers (gal4, gallery.hpp), which is exact, so the dot products run on the same f32 chain over widen(row).
// A chunk of at most 16 query rows may take the few-query phase 1 instead (topk_narrow_kernel, below): same bits, same order.
//
// Filtered search (MASKED instantiations of both phase-1 kernels): a device bitmap of uint32 words, row i
// allowed iff bit i & 31 of word i >> 5 is set, padded with zeros to whole 64-column tiles and 8-byte
// aligned (mask_eff_kernel builds it: live rows AND the caller's allow bits, bits >= N cleared).  A
// column whose bit is clear does not pass the ballot, so it never enters a list -- unlike a NaN score,
// which ranks below -inf but is an entry.  A span with no allowed row hands the merge k empty entries.
// The MASKED = false instantiations hold none of this: an unfiltered search launches them.
//
// Probabilities (PROBS instantiations of both phase-1 kernels and of the merge): the softmax over every row
// the search counts needs only a running (max, sum exp(l - max)) pair per query row, kept in registers where
// the scores already are, written once per (row, span) and combined in the merge, which then also writes
// exp(l - M) / S for the k results (or their sigmoid, which needs the merge alone).  ms_add / ms_group16
// below; the error bound is derived in DESIGN.md (embedding index, probabilities).  The PROBS = false
// instantiations keep no pair and write none.  Host side, at the end of the file: launch_topk checks its
// TopkArgs (kernels.hpp) and picks the phase-1 instantiation <KC, GT, MASKED, PROBS> from one table.
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "common.hpp"
#include "gallery.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_select.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

std::atomic<long> g_topk_span_cols{0};
std::atomic<int> g_topk_route{0};

namespace {

// (TB, TK, KQ, LDT, NB, the staging layout and the gallery element as loaded: topk_stage.hpp;
// CAND1, ent_key, ent_empty and compact_row: topk_select.hpp)
constexpr int CAND2 = 64;  // phase 2 (one ballot adds at most 64)
#ifndef CLIPGPU_TOPK_MERGE_STEPS
#define CLIPGPU_TOPK_MERGE_STEPS 4  // 64-entry steps the merge loads at once
#endif

// ---- softmax normaliser (PROBS instantiations) -----------------------------------------------------
// A row's running pair (m, s): m = the largest logit fed so far, s = sum exp(l - m) over them, by online
// rescaling: a logit above m rescales s by expf(m - l) and counts itself as 1, any other adds expf(l - m).
// Start: (-inf, 0).  A NaN logit makes s NaN for good (m ignores it); -inf adds nothing; +inf leaves
// m = +inf, which the merge turns into a NaN sum, as exp(inf - inf) does in softmax_rows_kernel.
__device__ __forceinline__ void ms_add(float& m, float& s, float l) {
  const bool up = l > m;
  const float a = expf(up ? m - l : l - m);  // one exp either way; unused for -inf against -inf (NaN)
  if (up) {
    s = s * a + 1.0f;
    m = l;
  } else if (l != -INFINITY) {
    s += a;
  }
}
// The pairs of the 16 lanes that share lane >> 4 (one accumulator row), as one pair: the maximum is exact,
// every lane rescales its sum once (by exactly 1 where it holds the maximum), then a fixed add tree.
__device__ __forceinline__ float2 ms_group16(float m, float s) {
  const float M = group16_max(m);
  return make_float2(M, group16_sum(m == M ? s : s * expf(m - M)));
}

// KC: list capacity the LDS is sized for (k <= KC); the LDS sets the blocks per CU (2 / 2 / 1 / 1 for
// KC 16 / 32 / 64 / 128), which the register budget follows.  Block: 64 queries x one gallery span.
// PROBS: every counted column's logit also feeds its row's (m, s); one pair per (row, span) goes to ms.
template <int KC, typename GT, bool MASKED, bool PROBS>
__global__ __launch_bounds__(256, KC <= 32 ? 2 : 1) void topk_partial_kernel(
    const float* __restrict__ qry, const GT* __restrict__ gal, int nq, int N, int E, float scale, float bias, int k,
    int span_cols, int n_spans, uint2* __restrict__ ws, const uint2* __restrict__ mask, float2* __restrict__ ms) {
  constexpr int STRIDE = KC + CAND1;
  __shared__ __attribute__((aligned(16))) float stage[2][TB * LDT];  // A | B: [row][k slot qd][k step]
  __shared__ uint2 sel[TB * STRIDE];
  __shared__ int cnt[TB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // blockIdx.x = query tile: the blocks of one span are dispatched together and share its rows in cache
  const int i0 = blockIdx.x * TB, span = blockIdx.y;
  // columns as unsigned: N < 2^31, but the last tile's padding columns may reach 2^31
  const unsigned c_begin = (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {
    // mask[t]: the two words of 64-column tile t.  A span with no allowed row (block-uniform): k empty
    // entries per query row, nothing staged.
    unsigned any = 0;
    for (unsigned t = (c_begin >> 6) + tid; t < ((c_end + 63) >> 6); t += 256) any |= mask[t].x | mask[t].y;
    if (!__syncthreads_or((int)(any != 0))) {
      for (int row = wave * 16; row < wave * 16 + 16; ++row)
        if (i0 + row < nq) {
          uint2* dst = ws + ((long)(i0 + row) * n_spans + span) * k;
          for (int t = lane; t < k; t += 64) dst[t] = ent_empty();
          if constexpr (PROBS)
            if (lane == 0) ms[(long)(i0 + row) * n_spans + span] = make_float2(-INFINITY, 0.f);
        }
      return;
    }
  }
  for (int i = tid; i < TB * STRIDE; i += 256) sel[i] = ent_empty();
  if (tid < TB) cnt[tid] = 0;
  __syncthreads();
  const int rowbase = wave * 16;
  const int r = lane & 15, qd = lane >> 4;
  uint64_t thr[4] = {0, 0, 0, 0};  // thresholds of rows rowbase + 4 * qd + e
  float pm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, ps[4] = {0.f, 0.f, 0.f, 0.f};  // PROBS: their (m, s)
  // Staging: a slab is 64 k = 16 MFMA steps.  Thread -> (rows tid / 16 + 16 p, p < 4; k step tid % 16):
  // one float4 = the four k slots of one step, 256 contiguous bytes per row across 16 threads.  In LDS
  // a row lies as [k slot qd][k step], so a lane's operands of four steps are one 16-byte read
  // (conflict-free with the strides KQ / LDT).  The next slab's loads (32 KiB per block) are issued
  // before this slab's 64 MFMAs per wave: with 16-k slabs the loop waited on memory latency.
  const int srow = tid >> 4, sj = tid & 15;
  auto load = [&](float4(&v)[4], const float* const(&src)[4], int k0) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      v[p] = k0 + sj * 4 < E ? *(const float4*)(src[p] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  // the gallery side stays as loaded (raw_t) until it is staged: widening it here would wait for the load
  typedef typename GalRaw<GT>::type raw_t;
  auto loadb = [&](raw_t(&v)[4], const GT* const(&src)[4], int k0) {
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = k0 + sj * 4 < E ? gal_raw(src[p] + k0) : raw_t{};  // zero bits widen to 0.f
  };
  auto put = [&](float* dst, const float4(&v)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float* d = dst + (p * 16 + srow) * LDT + sj;
      d[0] = v[p].x; d[KQ] = v[p].y; d[2 * KQ] = v[p].z; d[3 * KQ] = v[p].w;
    }
  };
  const float* pa[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pa[p] = qry + (long)min(i0 + p * 16 + srow, nq - 1) * E + sj * 4;
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
    float4 va[4];
    raw_t vb[4];
    load(va, pa, 0);
    loadb(vb, pb, 0);
    for (int k0 = 0; k0 < E; k0 += TK) {
      __syncthreads();
      put(stage[0], va);
      {
        float4 wb[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) wb[p] = gal_widen<GT>(vb[p]);
        put(stage[1], wb);
      }
      __syncthreads();
      if (k0 + TK < E) {
        load(va, pa, k0 + TK);
        loadb(vb, pb, k0 + TK);
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
    // C[row = 4 * qd + e][col = r] of column tile t
    if constexpr (PROBS) {
      // The counted columns (in range, allowed) feed their rows' pairs, ascending, whatever the thresholds
      // are; rows past nq keep pairs of their own that are never written.  A loop of its own: inside the
      // selection's it made that loop too large to unroll, and thr / pm / ps left the registers.
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          bool ok = j0 + t * 16 + r < c_end;
          if constexpr (MASKED) ok = ok && (((t < 2 ? mw.x : mw.y) >> ((t & 1) * 16 + r)) & 1u) != 0;
          if (ok) ms_add(pm[e], ps[e], fmaf(acc[t][e], scale, bias));
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned col = j0 + t * 16 + r;
        const uint32_t bits = __float_as_uint(fmaf(acc[t][e], scale, bias));
        const uint64_t key = topk_key(bits, col);
        bool ok = col < c_end;
        if constexpr (MASKED) ok = ok && (((t < 2 ? mw.x : mw.y) >> ((t & 1) * 16 + r)) & 1u) != 0;
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
  if constexpr (PROBS) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float2 p = ms_group16(pm[e], ps[e]);
      const int row = i0 + rowbase + 4 * qd + e;
      if (r == 0 && row < nq) ms[(long)row * n_spans + span] = p;
    }
  }
}

// One wave per query row: the k best of the row's n_spans * k partial results.
// PROBS (TOPK_PROBS_*): also out_prob [nq][k].  Softmax: the row's n_spans pairs give M (exact) and
// S = sum s_j exp(m_j - M), each lane adding its spans in ascending order, then a fixed add tree; the
// probability of an entry is expf(l - M) / S, (M, S) goes to out_norm if given.  Sigmoid: sigmoidf_ref of
// similarity.hip on the entry's logit.  Empty slots get 0.
template <int PROBS>
__global__ __launch_bounds__(256) void topk_merge_kernel(const uint2* __restrict__ ws, int nq, int n_spans, int k,
                                                         int64_t* __restrict__ out_idx, float* __restrict__ out_score,
                                                         const float2* __restrict__ ms, float* __restrict__ out_prob,
                                                         float* __restrict__ out_norm) {
  __shared__ uint2 sel[4][kTopkMax + CAND2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= nq) return;  // whole waves leave; the kernel has no block barrier
  uint2* ent = sel[wave];
  for (int t = lane; t < k; t += 64) ent[t] = ent_empty();
  wave_lds_order();
  const uint2* src = ws + (long)row * n_spans * k;
  const int total = n_spans * k;
  uint64_t thr = 0;
  int c = 0;
  // MS 64-entry steps are loaded at once: with few query rows this loop is one wave waiting on its own
  // loads.  They are processed in the order they lie in, so the selection runs as it did one step a time.
  // CLIPGPU_TOPK_MERGE_STEPS=1 (a variant build) is the one-step loop, for the A/B in DESIGN.md.
  constexpr int MS = CLIPGPU_TOPK_MERGE_STEPS;
  for (long base = 0; base < total; base += 64 * MS) {
    uint2 e4[MS];
#pragma unroll
    for (int u = 0; u < MS; ++u) {
      const long i = base + 64 * u + lane;
      e4[u] = i < total ? src[i] : ent_empty();
    }
#pragma unroll
    for (int u = 0; u < MS; ++u) {
      const uint2 e = e4[u];
      const uint64_t key = ent_key(e);
      bool pass = key > thr;  // an empty entry (key 0) never passes
      uint64_t bal = __ballot(pass);
      if (bal == 0) continue;
      if (c + __popcll(bal) > CAND2) {
        thr = compact_row(ent, k, c, lane);
        c = 0;
        pass = key > thr;
        bal = __ballot(pass);
      }
      if (pass) ent[k + c + __popcll(bal & ((1ull << lane) - 1ull))] = e;
      wave_lds_order();
      c += __popcll(bal);
    }
  }
  if (c > 0) compact_row(ent, k, c, lane);
  float M = -INFINITY, S = 0.f;
  if constexpr (PROBS == TOPK_PROBS_SOFTMAX) {
    const float2* pr = ms + (long)row * n_spans;
    for (int j = lane; j < n_spans; j += 64) M = fmaxf(M, pr[j].x);
    M = wave_max(M);
    for (int j = lane; j < n_spans; j += 64) {
      const float2 p = pr[j];
      S += p.x == M ? p.y : p.y * expf(p.x - M);
    }
    S = wave_sum(S);
    if (M == INFINITY) S = NAN;  // exp(inf - inf)
    if (out_norm && lane == 0) {
      out_norm[2 * (long)row] = M;
      out_norm[2 * (long)row + 1] = S;
    }
  }
  for (int t = lane; t < k; t += 64) {
    const uint2 e = ent[t];
    const bool empty = e.y == kTopkEmptyIndex;
    out_idx[(long)row * k + t] = empty ? -1 : (int64_t)e.y;
    out_score[(long)row * k + t] = empty ? -INFINITY : __uint_as_float(e.x);
    if constexpr (PROBS == TOPK_PROBS_SOFTMAX)
      out_prob[(long)row * k + t] = empty ? 0.f : expf(__uint_as_float(e.x) - M) / S;
    if constexpr (PROBS == TOPK_PROBS_SIGMOID)
      out_prob[(long)row * k + t] = empty ? 0.f : 1.0f / (1.0f + expf(-__uint_as_float(e.x)));
  }
}

// ---- few queries: at most 16 query rows per launch -------------------------------------------------
// The wide kernel's 64-row query tile does 64 / nq times the MFMA work a few queries need, and its two
// blocks per CU stream the gallery at a fraction of the HBM rate.  Here a block is ONE wave that owns a
// 16-row query tile and a gallery span, walked in 16-column tiles: one 16x16 MFMA tile, the same
// v_mfma_f32_16x16x4_f32 chain in the same k order through the same [k slot][k step] staging, so the
// scores carry the wide kernel's bits.  There is no block barrier: the wave stages into LDS of its own
// (11 KiB) and keeps its rows' selection state (16 x (KC + 32) entries), 17 - 32 KiB per block, so 9 to 5
// waves per CU are resident.  Slabs of 64 k are requested two ahead, into registers, in one flat
// sequence over (tile, slab): the loads of the next tile are in flight during this tile's MFMAs and
// selection (up to 2 x 4 KiB of gallery per wave for f32, 2 x 2 KiB for 16-bit; see request() for what
// the compiled loop keeps of it).  Query rows past nq are
// clamped for the loads and never enter the selection.
//
// MASKED: the allowed bits of a 16-column tile are half a mask word.  Every request carries one more
// load, the word of the tile it requests (a request is still the same loads whatever the position), so
// the word arrives with the tile's last slab and the selection starts no load of its own.  A tile is
// never skipped -- a conditional request would end the counting of the loads in flight; only a span
// with no allowed row leaves at once.
//
// PROBS: as in the wide kernel; the columns of the step past the span are all >= c_end and are not counted.
template <int KC, typename GT, bool MASKED, bool PROBS>
__global__ __launch_bounds__(64) void topk_narrow_kernel(const float* __restrict__ qry, const GT* __restrict__ gal,
                                                         int nq, int N, int E, float scale, float bias, int k,
                                                         int span_cols, int n_spans, uint2* __restrict__ ws,
                                                         const uint32_t* __restrict__ mask, float2* __restrict__ ms) {
  typedef typename GalRaw<GT>::type raw_t;
  constexpr int STRIDE = KC + CAND1;
  __shared__ __attribute__((aligned(16))) float stage[2][NB * LDT];  // A | B: [row][k slot qd][k step]
  __shared__ uint2 sel[NB * STRIDE];
  __shared__ int cnt[NB];
  const int lane = threadIdx.x, span = blockIdx.x;
  const unsigned c_begin = (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {  // a span with no allowed row: k empty entries per query row, nothing requested
    unsigned any = 0;
    for (unsigned w = (c_begin >> 5) + lane; w < ((c_end + 63) >> 6) * 2; w += 64) any |= mask[w];
    if (__ballot(any != 0) == 0) {
      for (int row = 0; row < nq; ++row) {
        uint2* dst = ws + ((long)row * n_spans + span) * k;
        for (int t = lane; t < k; t += 64) dst[t] = ent_empty();
        if constexpr (PROBS)
          if (lane == 0) ms[(long)row * n_spans + span] = make_float2(-INFINITY, 0.f);
      }
      return;
    }
  }
  for (int i = lane; i < NB * STRIDE; i += 64) sel[i] = ent_empty();
  if (lane < NB) cnt[lane] = 0;
  wave_lds_order();
  const int r = lane & 15, qd = lane >> 4;
  uint64_t thr[4] = {0, 0, 0, 0};  // thresholds of rows 4 * qd + e
  float pm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, ps[4] = {0.f, 0.f, 0.f, 0.f};  // PROBS: their (m, s)
  // Staging as in the wide kernel, by one wave: lane -> (rows lane / 16 + 4 p, p < 4; k step lane % 16).
  const int srow = lane >> 4, sj = lane & 15;
  const float* pa[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pa[p] = qry + (long)min(p * 4 + srow, nq - 1) * E;
  unsigned lj = c_begin;  // the next slab to request: tile lj, k lk
  int lk = 0;
  // Every request is the same eight loads, whatever the position, so that the compiler can count the
  // loads in flight (with a conditional request it waits for all of them at every step).  In the ISA the
  // second step of the pair below waits with eight loads left in flight (vmcnt(8)) and the first with
  // six (f32) or four (16-bit): not the full slab there, because the compiler reorders the loads of the
  // prologue, but no step waits for all of them any more.
  // A lane whose k step lies past the end of E reads the
  // row's last four elements instead (the MFMA loop never reads what it stages: it stops at E); past
  // the end of the span the request reads the gallery's last rows again and nobody uses it.
  auto request = [&](float4(&va)[4], raw_t(&vb)[4], uint32_t& vm) {
    const int ko = min(lk + sj * 4, E - 4);
    // The word of tile lj, first: the oldest load of the request.  lj + 4 * srow lies in the tile, so
    // every lane reads the same word; formed from the lane's row the address is not uniform to the
    // compiler and the load is a vector load, counted with the eight below.
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
  // C[row = 4 * qd + e][col = r] of the tile at column cj: the wide kernel's selection, on one column tile.
  // The ballot / compact / append block is written out a second time on purpose: one shared __forceinline__
  // function for both kernels was tried and changes the generated code of nearly every instantiation.
  auto select = [&](unsigned cj, const f32x4& acc, bool allowed) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e >= nq) break;  // rows 4 * qd + e >= e: all padding
      const unsigned col = cj + r;
      const int rl = 4 * qd + e;
      const uint32_t bits = __float_as_uint(fmaf(acc[e], scale, bias));
      const uint64_t key = topk_key(bits, col);
      const bool live = col < c_end && rl < nq && allowed;
      if constexpr (PROBS)  // rows past nq keep pairs of their own, never written
        if (col < c_end && allowed) ms_add(pm[e], ps[e], __uint_as_float(bits));
      bool pass = live && key > thr[e];
      uint64_t bal = __ballot(pass);
      if (bal == 0) continue;
      unsigned mq = (unsigned)(bal >> (16 * qd)) & 0xffffu;
      int c = cnt[rl];
      if (__ballot(c + __popc(mq) > CAND1) != 0) {
        for (int g = 0; g < 4; ++g) {  // the four rows this ballot covers
          const int row = 4 * g + e;
          const int c2 = cnt[row];
          if (c2 + __popc((unsigned)(bal >> (16 * g)) & 0xffffu) > CAND1) {
            const uint64_t t2 = compact_row(sel + row * STRIDE, k, c2, lane);
            if (lane == 0) cnt[row] = 0;
            if (qd == g) thr[e] = t2;
          }
        }
        wave_lds_order();
        pass = live && key > thr[e];
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
  unsigned cj = c_begin;  // the slab in hand: tile cj, k ck
  int ck = 0;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step = [&](float4(&va)[4], raw_t(&vb)[4], uint32_t& vm) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      put(stage[0], p, va[p]);
      put(stage[1], p, gal_widen<GT>(vb[p]));
    }
    // The bit of column cj + r (the tile is the low or the high half of its word), taken here: the word
    // arrived before the rows just staged, and its register is free again for the request below.  Held
    // across the request instead, the word's next value needs a second register and a copy at the end of
    // the loop, which waits for every load.
    // (The empty asm keeps the compiler from moving the shift down to the selection, past the request.)
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
  // The steps run in pairs, a fixed number of them, with no exit between the two of a pair: with an exit
  // there the compiler sees a path from one first step to the next without the second one's loads and
  // waits for every load.  An odd count ends in one step past the span: it stages rows that request()
  // clamped into the gallery, and if it completes a tile, every column of it is >= c_end and none passes.
  // The barriers keep the two prologue requests apart, so that the first step's loads are the older ones.
  request(a0, b0, m0);
  __builtin_amdgcn_sched_barrier(0);
  request(a1, b1, m1);
  __builtin_amdgcn_sched_barrier(0);
  const int n_steps = (int)((c_end - c_begin + NB - 1) / NB) * ((E + TK - 1) / TK);
  for (int it = 0; it < n_steps; it += 2) {
    step(a0, b0, m0);
    step(a1, b1, m1);
  }
  for (int row = 0; row < nq; ++row) {
    const int c2 = cnt[row];
    if (c2 > 0) compact_row(sel + row * STRIDE, k, c2, lane);
    uint2* dst = ws + ((long)row * n_spans + span) * k;
    for (int t = lane; t < k; t += 64) dst[t] = sel[row * STRIDE + t];
  }
  if constexpr (PROBS) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float2 p = ms_group16(pm[e], ps[e]);
      if (r == 0 && 4 * qd + e < nq) ms[(long)(4 * qd + e) * n_spans + span] = p;
    }
  }
}

// eff[w] = live[w] & allow[w] for the words that hold rows [0, n), bits >= n cleared, zeros up to the end
// of the last 64-column tile.  live / allow NULL = all ones; both are read in their first ceil(n / 32)
// words only.  allow may be eff itself (each thread reads and writes its own word).
__global__ __launch_bounds__(256) void mask_eff_kernel(const uint32_t* live, const uint32_t* allow, uint32_t* eff,
                                                       long n, long words) {
  for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < words; w += (long)gridDim.x * 256) {
    uint32_t v = 0;
    if (w * 32 < n) {
      v = (live ? live[w] : ~0u) & (allow ? allow[w] : ~0u);
      if (n - w * 32 < 32) v &= (1u << (n - w * 32)) - 1u;
    }
    eff[w] = v;
  }
}

// ---- launches: phase 1 of one instantiation, the few-query kernel or the wide one as the plan says ----
template <int KC, typename GT, bool MASKED, bool PROBS>
void launch_phase1(const TopkArgs& a, float2* ms) {
  const TopkPlan& p = a.plan;
  if (p.narrow)
    hipLaunchKernelGGL((topk_narrow_kernel<KC, GT, MASKED, PROBS>), dim3(p.n_spans), dim3(64), 0, a.stream, a.q,
                       (const GT*)a.g, a.nq, a.N, a.E, a.scale, a.bias, a.k, p.span_cols, p.n_spans, (uint2*)a.ws, a.mask,
                       ms);
  else
    hipLaunchKernelGGL((topk_partial_kernel<KC, GT, MASKED, PROBS>), dim3((a.nq + TB - 1) / TB, p.n_spans), dim3(256), 0,
                       a.stream, a.q, (const GT*)a.g, a.nq, a.N, a.E, a.scale, a.bias, a.k, p.span_cols, p.n_spans,
                       (uint2*)a.ws, (const uint2*)a.mask, ms);
}

// Every instantiation: [gallery type][MASKED][PROBS][list capacity 16 / 32 / 64 / 128].
typedef void (*Phase1)(const TopkArgs&, float2*);
#define PHASE1_KC(GT, M, P) \
  { launch_phase1<16, GT, M, P>, launch_phase1<32, GT, M, P>, launch_phase1<64, GT, M, P>, launch_phase1<128, GT, M, P> }
#define PHASE1_GT(GT) \
  { {PHASE1_KC(GT, false, false), PHASE1_KC(GT, false, true)}, {PHASE1_KC(GT, true, false), PHASE1_KC(GT, true, true)} }
constexpr Phase1 kPhase1[3][2][2][4] = {PHASE1_GT(float), PHASE1_GT(_Float16), PHASE1_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kPhase1");

// The smallest list capacity that holds k, MASKED iff there is a mask, PROBS iff there are pairs to write (ms).
void dispatch_phase1(const TopkArgs& a, float2* ms) {
  const int kc = a.k <= 16 ? 0 : a.k <= 32 ? 1 : a.k <= 64 ? 2 : 3;
  kPhase1[a.dtype][a.mask != nullptr][ms != nullptr][kc](a, ms);
}

// Phase 2; the outputs an instantiation does not write are passed as NULL.
template <int PROBS>
void launch_merge(const TopkArgs& a, const float2* ms) {
  hipLaunchKernelGGL(topk_merge_kernel<PROBS>, dim3((a.nq + 3) / 4), dim3(256), 0, a.stream, (const uint2*)a.ws, a.nq,
                     a.plan.n_spans, a.k, a.out_idx, a.out_score, ms, PROBS == TOPK_PROBS_NONE ? nullptr : a.out_prob,
                     PROBS == TOPK_PROBS_SOFTMAX ? a.out_norm : nullptr);
}

}  // namespace

long topk_mask_words(long n) { return (n + 63) / 64 * 2; }

hipError_t launch_topk_mask(const uint32_t* live, const uint32_t* allow, uint32_t* eff, long n, hipStream_t s) {
  if (n <= 0 || !eff) return hipErrorInvalidValue;
  const long words = topk_mask_words(n);
  hipLaunchKernelGGL(mask_eff_kernel, dim3((int)std::min<long>((words + 255) / 256, 1024)), dim3(256), 0, s, live, allow,
                     eff, n, words);
  return hipGetLastError();
}

bool topk_narrow_route(int nq) {
  const int route = g_topk_route.load();
  if (route == 1 || nq > NB) return false;
  return route == 2 || nq <= kNarrowRows;
}

TopkPlan topk_plan(long N, int nq, int max_blocks) {
  const long tiles = (N + TB - 1) / TB;
  TopkPlan p;
  p.narrow = topk_narrow_route(nq);
  // spans the workspace holds: it is sized for max_blocks blocks of 64 query rows, a narrow launch has 16
  const long most = p.narrow ? std::min<long>(4L * max_blocks, kNarrowSpans) : std::max(1L, (long)max_blocks / ((nq + TB - 1) / TB));
  long want = std::min(tiles, most);
  const long forced = g_topk_span_cols.load();
  if (forced > 0) want = std::min(most, (tiles + forced / TB - 1) / (forced / TB));
  p.span_cols = (int)((tiles + want - 1) / want) * TB;
  p.n_spans = (int)((N + p.span_cols - 1) / p.span_cols);
  return p;
}

hipError_t launch_topk_merge(const void* ws, int nq, int n_spans, int k, int64_t* out_idx, float* out_score,
                             hipStream_t s) {
  if (!ws || !out_idx || !out_score || nq <= 0 || n_spans <= 0 || n_spans > 65535 || k < 1 || k > kTopkMax ||
      (long)n_spans * k > INT32_MAX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(topk_merge_kernel<TOPK_PROBS_NONE>, dim3((nq + 3) / 4), dim3(256), 0, s, (const uint2*)ws, nq,
                     n_spans, k, out_idx, out_score, (const float2*)nullptr, (float*)nullptr, (float*)nullptr);
  return hipGetLastError();
}

hipError_t launch_topk(const TopkArgs& a) {
  const TopkPlan& p = a.plan;
  if (a.nq <= 0 || a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.k < 1 || a.k > kTopkMax) return hipErrorInvalidValue;
  if (p.span_cols <= 0 || p.span_cols % TB != 0 || (long)p.n_spans * p.span_cols < a.N ||
      (long)(p.n_spans - 1) * p.span_cols >= a.N || (long)p.n_spans * a.k > INT32_MAX || p.n_spans > 65535)
    return hipErrorInvalidValue;
  if (p.narrow && a.nq > NB) return hipErrorInvalidValue;
  if (a.mask && ((uintptr_t)a.mask & 7)) return hipErrorInvalidValue;
  if (a.probs < TOPK_PROBS_NONE || a.probs > TOPK_PROBS_SIGMOID) return hipErrorInvalidValue;
  if (a.probs != TOPK_PROBS_NONE && !a.out_prob) return hipErrorInvalidValue;
  // softmax: one (m, s) pair per (query row, span) in a.ms
  float2* ms = a.probs == TOPK_PROBS_SOFTMAX ? (float2*)a.ms : nullptr;
  if (a.probs == TOPK_PROBS_SOFTMAX && (!ms || ((uintptr_t)ms & 7) || (long)a.nq * p.n_spans > a.ms_pairs))
    return hipErrorInvalidValue;
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  dispatch_phase1(a, ms);
  if (a.probs == TOPK_PROBS_SOFTMAX) launch_merge<TOPK_PROBS_SOFTMAX>(a, ms);
  else if (a.probs == TOPK_PROBS_SIGMOID) launch_merge<TOPK_PROBS_SIGMOID>(a, nullptr);
  else launch_merge<TOPK_PROBS_NONE>(a, nullptr);
  return hipGetLastError();
}

}  // namespace clipgpu
