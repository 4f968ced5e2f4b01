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
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"

namespace clipgpu {

std::atomic<long> g_topk_span_cols{0};

namespace {

constexpr int TB = 64, TK = 64;
constexpr int KQ = 20, LDT = 88;  // staged row: 4 k slots of 16 steps + 4, + 8: conflict-free 16-byte reads
constexpr int CAND1 = 32;  // phase 1 candidate slots per row (one ballot adds at most 16 to a row)
constexpr int CAND2 = 64;  // phase 2 (one ballot adds at most 64)

// A selection entry: x = the score's own f32 bits, y = gallery index.  Compared by topk_key.
__device__ __forceinline__ uint64_t ent_key(uint2 e) { return topk_key(e.x, e.y); }
__device__ __forceinline__ uint2 ent_empty() { return make_uint2(kTopkEmptyScore, kTopkEmptyIndex); }

// LDS traffic of one wave is processed in program order; this keeps the compiler from moving it.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Wave-cooperative (all 64 lanes, uniform arguments).  ent[0 .. k) is the row's current best list,
// ent[k .. k + c) its candidates (k + c <= 192).  Leaves the k best of both in ent[0 .. k), best
// first, and returns the key of ent[k - 1]: the row's new threshold (0 while the list has empty
// slots).  Empty entries all have key 0; the position breaks that tie, so ranks are a permutation.
__device__ __forceinline__ uint64_t compact_row(uint2* ent, int k, int c, int lane) {
  const int m = k + c;
  uint2 mine[3];
  uint64_t mk[3];
  int rank[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int i = lane + 64 * s;
    mine[s] = i < m ? ent[i] : ent_empty();
    mk[s] = ent_key(mine[s]);
    rank[s] = 0;
  }
  for (int j = 0; j < m; ++j) {
    const uint64_t kj = ent_key(ent[j]);  // same address in every lane: an LDS broadcast
#pragma unroll
    for (int s = 0; s < 3; ++s)
      if (64 * s < m) rank[s] += (kj > mk[s] || (kj == mk[s] && j < lane + 64 * s)) ? 1 : 0;
  }
  wave_lds_order();
#pragma unroll
  for (int s = 0; s < 3; ++s)
    if (lane + 64 * s < m && rank[s] < k) ent[rank[s]] = mine[s];
  wave_lds_order();
  return ent_key(ent[k - 1]);
}

// KC: list capacity the LDS is sized for (k <= KC); the LDS sets the blocks per CU (2 / 2 / 1 / 1 for
// KC 16 / 32 / 64 / 128), which the register budget follows.  Block: 64 queries x one gallery span.
template <int KC>
__global__ __launch_bounds__(256, KC <= 32 ? 2 : 1) void topk_partial_kernel(
    const float* __restrict__ qry, const float* __restrict__ gal, int nq, int N, int E, float scale, float bias, int k,
    int span_cols, int n_spans, uint2* __restrict__ ws) {
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
  for (int i = tid; i < TB * STRIDE; i += 256) sel[i] = ent_empty();
  if (tid < TB) cnt[tid] = 0;
  __syncthreads();
  const int rowbase = wave * 16;
  const int r = lane & 15, qd = lane >> 4;
  uint64_t thr[4] = {0, 0, 0, 0};  // thresholds of rows rowbase + 4 * qd + e
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
    const float* pb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) pb[p] = gal + (long)min(j0 + p * 16 + srow, (unsigned)N - 1) * E + sj * 4;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 va[4], vb[4];
    load(va, pa, 0);
    load(vb, pb, 0);
    for (int k0 = 0; k0 < E; k0 += TK) {
      __syncthreads();
      put(stage[0], va);
      put(stage[1], vb);
      __syncthreads();
      if (k0 + TK < E) {
        load(va, pa, k0 + TK);
        load(vb, pb, k0 + TK);
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
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned col = j0 + t * 16 + r;
        const uint32_t bits = __float_as_uint(fmaf(acc[t][e], scale, bias));
        const uint64_t key = topk_key(bits, col);
        bool pass = col < c_end && key > thr[e];
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
          pass = col < c_end && key > thr[e];
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
}

// One wave per query row: the k best of the row's n_spans * k partial results.
__global__ __launch_bounds__(256) void topk_merge_kernel(const uint2* __restrict__ ws, int nq, int n_spans, int k,
                                                         int64_t* __restrict__ out_idx, float* __restrict__ out_score) {
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
  for (int base = 0; base < total; base += 64) {
    const int i = base + lane;
    const uint2 e = i < total ? src[i] : ent_empty();
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
  if (c > 0) compact_row(ent, k, c, lane);
  for (int t = lane; t < k; t += 64) {
    const uint2 e = ent[t];
    const bool empty = e.y == kTopkEmptyIndex;
    out_idx[(long)row * k + t] = empty ? -1 : (int64_t)e.y;
    out_score[(long)row * k + t] = empty ? -INFINITY : __uint_as_float(e.x);
  }
}

template <int KC>
void launch_partial(const float* q, int nq, const float* g, int N, int E, float scale, float bias, int k,
                    const TopkPlan& p, void* ws, hipStream_t s) {
  hipLaunchKernelGGL(topk_partial_kernel<KC>, dim3((nq + TB - 1) / TB, p.n_spans), dim3(256), 0, s, q, g, nq, N, E,
                     scale, bias, k, p.span_cols, p.n_spans, (uint2*)ws);
}

}  // namespace

TopkPlan topk_plan(long N, int q_tiles, int max_blocks) {
  const long tiles = (N + TB - 1) / TB;
  const long most = std::max(1L, (long)max_blocks / q_tiles);  // spans the workspace holds
  long want = std::min(tiles, most);
  const long forced = g_topk_span_cols.load();
  if (forced > 0) want = std::min(most, (tiles + forced / TB - 1) / (forced / TB));
  TopkPlan p;
  p.span_cols = (int)((tiles + want - 1) / want) * TB;
  p.n_spans = (int)((N + p.span_cols - 1) / p.span_cols);
  return p;
}

hipError_t launch_topk(const float* q, int nq, const float* g, int N, int E, float scale, float bias, int k,
                       const TopkPlan& p, void* ws, int64_t* out_idx, float* out_score, hipStream_t s) {
  if (nq <= 0 || N <= 0 || E <= 0 || E % 16 != 0 || k < 1 || k > kTopkMax) return hipErrorInvalidValue;
  if (p.span_cols <= 0 || p.span_cols % TB != 0 || (long)p.n_spans * p.span_cols < N ||
      (long)(p.n_spans - 1) * p.span_cols >= N || (long)p.n_spans * k > INT32_MAX || p.n_spans > 65535)
    return hipErrorInvalidValue;
  if (k <= 16) launch_partial<16>(q, nq, g, N, E, scale, bias, k, p, ws, s);
  else if (k <= 32) launch_partial<32>(q, nq, g, N, E, scale, bias, k, p, ws, s);
  else if (k <= 64) launch_partial<64>(q, nq, g, N, E, scale, bias, k, p, ws, s);
  else launch_partial<128>(q, nq, g, N, E, scale, bias, k, p, ws, s);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, (const uint2*)ws, nq, p.n_spans, k,
                     out_idx, out_score);
  return hipGetLastError();
}

}  // namespace clipgpu
