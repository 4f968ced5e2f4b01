// Range search of a device-resident gallery (clipgpu_index_range_search, clipgpu_index_self_join): every
// gallery row whose score against a query is at or above a threshold, without the [n_q][N] score matrix.
//
//   score[i][j] = fmaf(dot(q[i], g[j]), scale, bias)        bit-identical to sim_logits_kernel and to the search
//   hit         = j in range, live and allowed, score >= threshold as f32 (a NaN score never passes)
//
// The two kernels are phase 1 of the top-k search (kernels/topk.hip) with the selection taken out: the same
// 64-query tile against gallery spans (range_wide_kernel, as topk_partial_kernel) and the same one-wave
// 16-row tile (range_narrow_kernel, as topk_narrow_kernel), the same v_mfma_f32_16x16x4_f32 chain in the
// same k order through the same [k slot][k step] staging (topk_stage.hpp), so a score carries the search's
// bits.  There is no per-row list, no candidate buffer, no compaction and no merge: the LDS is the staging
// alone (44 KiB wide, 11 KiB few-query).
//
// Emission.  After a tile's MFMAs every lane holds its hits as bits of one register.  A wave ballot of
// "any hit" is zero for nearly every tile and then nothing more happens.  Otherwise the lanes' hit counts
// are summed and prefix-summed over the wave with one ballot per bit of the count, lane 0 adds the wave's
// sum to the 64-bit global counter (one atomic per wave and tile, however many hits), the base is
// broadcast, and every lane writes its records at base + prefix + 0, 1, ... -- each only if that position
// is below the capacity.  The counter keeps counting past the capacity, so the caller learns the exact
// total.  A record is three 4-byte stores into three arrays (query, row, score): the C ABI's device form
// hands them out as they are.
//
// Self-join (the `join` launch parameter, not another kernel family): the query rows are gallery rows
// q_off .. q_off + nq, a column j passes for query row i only if j > i and row i itself is allowed (a
// second test against the same bitmap), and the spans start at col0 = q_off & ~63.
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

// v of the first lane in every lane (all lanes active: the first is lane 0)
__device__ __forceinline__ unsigned long long wave_first(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

struct RangeOut {
  int32_t* query;
  int32_t* row;
  float* score;
  unsigned long long* total;
  unsigned long long capacity;
};

// Wave-cooperative (all 64 lanes): lane `lane` has n <= 2^BITS - 1 hits.  Adds the wave's hits to the
// counter and returns the position of this lane's first one.
template <int BITS>
__device__ __forceinline__ unsigned long long wave_reserve(const RangeOut& o, int n, int lane) {
  const uint64_t below = (1ull << lane) - 1ull;
  unsigned pre = 0, sum = 0;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const uint64_t bb = __ballot((n >> b) & 1);
    pre += (unsigned)__popcll(bb & below) << b;
    sum += (unsigned)__popcll(bb) << b;
  }
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(o.total, (unsigned long long)sum);
  return wave_first(base) + pre;
}

__device__ __forceinline__ void put_record(const RangeOut& o, unsigned long long pos, int query, unsigned col, float s) {
  if (pos < o.capacity) {
    o.query[pos] = query;
    o.row[pos] = (int32_t)col;
    o.score[pos] = s;
  }
}

// Block: 64 queries x one gallery span, as topk_partial_kernel.  44 KiB of LDS: three blocks per CU.
template <typename GT, bool MASKED>
__global__ __launch_bounds__(256, 3) void range_wide_kernel(const float* __restrict__ qry, const GT* __restrict__ gal,
                                                            int nq, int N, int E, float scale, float bias, float thr,
                                                            unsigned col0, int span_cols,
                                                            const uint2* __restrict__ mask, int q_off, bool join,
                                                            RangeOut out) {
  __shared__ __attribute__((aligned(16))) float stage[2][TB * LDT];  // A | B: [row][k slot qd][k step]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * TB, span = blockIdx.y;
  // columns as unsigned: N < 2^31, but the last tile's padding columns may reach 2^31
  const unsigned c_begin = col0 + (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {  // a span with no allowed row (block-uniform): nothing to do
    unsigned any = 0;
    for (unsigned t = (c_begin >> 6) + tid; t < ((c_end + 63) >> 6); t += 256) any |= mask[t].x | mask[t].y;
    if (!__syncthreads_or((int)(any != 0))) return;
  }
  const int rowbase = wave * 16;
  const int r = lane & 15, qd = lane >> 4;
  // rows rowbase + 4 * qd + e: their query indices, and whether they can have a hit at all (inside the
  // batch; self-join: the row itself live and allowed)
  int qi[4];
  bool rowok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = i0 + rowbase + 4 * qd + e;
    qi[e] = q_off + row;
    rowok[e] = row < nq;
    if constexpr (MASKED)
      if (join && rowok[e]) rowok[e] = ((((const uint32_t*)mask)[qi[e] >> 5] >> (qi[e] & 31)) & 1u) != 0;
  }
  // Staging: as topk_partial_kernel (thread -> rows tid / 16 + 16 p, k step tid % 16; the next slab's loads
  // are issued before this slab's MFMAs).
  const int srow = tid >> 4, sj = tid & 15;
  auto load = [&](float4(&v)[4], const float* const(&src)[4], int k0) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      v[p] = k0 + sj * 4 < E ? *(const float4*)(src[p] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
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
    // self-join: every column of the tile is at or below every query row of the block (block-uniform)
    if (join && j0 + (TB - 1) <= (unsigned)(q_off + i0)) continue;
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
    // C[row = 4 * qd + e][col = r] of column tile t; hit bit 4 * e + t
    unsigned hit = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned col = j0 + t * 16 + r;
        bool ok = col < c_end && rowok[e];
        if constexpr (MASKED) ok = ok && (((t < 2 ? mw.x : mw.y) >> ((t & 1) * 16 + r)) & 1u) != 0;
        if (join) ok = ok && col > (unsigned)qi[e];
        if (ok && fmaf(acc[t][e], scale, bias) >= thr) hit |= 1u << (4 * e + t);
      }
    if (__ballot(hit != 0) == 0) continue;  // wave-uniform: the common case
    unsigned long long pos = wave_reserve<5>(out, __popc(hit), lane);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if ((hit >> (4 * e + t)) & 1u) put_record(out, pos++, qi[e], j0 + t * 16 + r, fmaf(acc[t][e], scale, bias));
  }
}

// One wave: a 16-row query tile against a gallery span in 16-column tiles, as topk_narrow_kernel -- the
// same flat sequence of requests two slabs ahead (see there for why every request is the same loads and
// why the steps run in pairs), and no block barrier.  11 KiB of LDS.
template <typename GT, bool MASKED>
__global__ __launch_bounds__(64) void range_narrow_kernel(const float* __restrict__ qry, const GT* __restrict__ gal,
                                                          int nq, int N, int E, float scale, float bias, float thr,
                                                          unsigned col0, int span_cols,
                                                          const uint32_t* __restrict__ mask, int q_off, bool join,
                                                          RangeOut out) {
  typedef typename GalRaw<GT>::type raw_t;
  __shared__ __attribute__((aligned(16))) float stage[2][NB * LDT];  // A | B: [row][k slot qd][k step]
  const int lane = threadIdx.x, span = blockIdx.x;
  const unsigned c_begin = col0 + (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {  // a span with no allowed row: nothing requested
    unsigned any = 0;
    for (unsigned w = (c_begin >> 5) + lane; w < ((c_end + 63) >> 6) * 2; w += 64) any |= mask[w];
    if (__ballot(any != 0) == 0) return;
  }
  const int r = lane & 15, qd = lane >> 4;
  int qi[4];  // rows 4 * qd + e, as in the wide kernel
  bool rowok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = 4 * qd + e;
    qi[e] = q_off + row;
    rowok[e] = row < nq;
    if constexpr (MASKED)
      if (join && rowok[e]) rowok[e] = ((mask[qi[e] >> 5] >> (qi[e] & 31)) & 1u) != 0;
  }
  // Staging as in the wide kernel, by one wave: lane -> (rows lane / 16 + 4 p, p < 4; k step lane % 16).
  const int srow = lane >> 4, sj = lane & 15;
  const float* pa[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pa[p] = qry + (long)min(p * 4 + srow, nq - 1) * E;
  unsigned lj = c_begin;  // the next slab to request: tile lj, k lk
  int lk = 0;
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
  // C[row = 4 * qd + e][col = r] of the tile at column cj; hit bit e
  auto emit = [&](unsigned cj, const f32x4& acc, bool allowed) {
    const unsigned col = cj + r;
    unsigned hit = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool ok = col < c_end && rowok[e] && allowed;
      if (join) ok = ok && col > (unsigned)qi[e];
      if (ok && fmaf(acc[e], scale, bias) >= thr) hit |= 1u << e;
    }
    if (__ballot(hit != 0) == 0) return;  // wave-uniform: the common case
    unsigned long long pos = wave_reserve<3>(out, __popc(hit), lane);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if ((hit >> e) & 1u) put_record(out, pos++, qi[e], col, fmaf(acc[e], scale, bias));
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
    // the bit of column cj + r, taken before the request reuses the word's register (topk_narrow_kernel)
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
      emit(cj, acc, allowed);
      acc = f32x4{0.f, 0.f, 0.f, 0.f};
      ck = 0;
      cj += NB;
    }
  };
  float4 a0[4] = {}, a1[4] = {};
  raw_t b0[4] = {}, b1[4] = {};
  uint32_t m0 = 0, m1 = 0;
  // An odd count of steps ends in one step past the span: it stages rows that request() clamped into the
  // gallery, and if it completes a tile, every column of it is >= c_end and none passes.
  request(a0, b0, m0);
  __builtin_amdgcn_sched_barrier(0);
  request(a1, b1, m1);
  __builtin_amdgcn_sched_barrier(0);
  const int n_steps = (int)((c_end - c_begin + NB - 1) / NB) * ((E + TK - 1) / TK);
  for (int it = 0; it < n_steps; it += 2) {
    step(a0, b0, m0);
    step(a1, b1, m1);
  }
}

template <typename GT, bool MASKED>
void launch_range_of(const RangeArgs& a) {
  const TopkPlan& p = a.plan;
  const RangeOut out = {a.out_query, a.out_row, a.out_score, a.total, (unsigned long long)a.capacity};
  if (p.narrow)
    hipLaunchKernelGGL((range_narrow_kernel<GT, MASKED>), dim3(p.n_spans), dim3(64), 0, a.stream, a.q, (const GT*)a.g,
                       a.nq, a.N, a.E, a.scale, a.bias, a.threshold, a.col0, p.span_cols, a.mask, a.q_off, a.join, out);
  else
    hipLaunchKernelGGL((range_wide_kernel<GT, MASKED>), dim3((a.nq + TB - 1) / TB, p.n_spans), dim3(256), 0, a.stream,
                       a.q, (const GT*)a.g, a.nq, a.N, a.E, a.scale, a.bias, a.threshold, a.col0, p.span_cols,
                       (const uint2*)a.mask, a.q_off, a.join, out);
}

// Every instantiation: [gallery type][MASKED].
typedef void (*RangeLaunch)(const RangeArgs&);
#define RANGE_GT(GT) { launch_range_of<GT, false>, launch_range_of<GT, true> }
constexpr RangeLaunch kRange[3][2] = {RANGE_GT(float), RANGE_GT(_Float16), RANGE_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kRange");

}  // namespace

hipError_t launch_range(const RangeArgs& a) {
  const TopkPlan& p = a.plan;
  if (a.nq <= 0 || a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.q_off < 0) return hipErrorInvalidValue;
  if (a.col0 % TB != 0 || a.col0 >= (unsigned)a.N) return hipErrorInvalidValue;
  const long cols = (long)a.N - a.col0;  // the columns the spans cover
  if (p.span_cols <= 0 || p.span_cols % TB != 0 || (long)p.n_spans * p.span_cols < cols ||
      (long)(p.n_spans - 1) * p.span_cols >= cols || p.n_spans > 65535)
    return hipErrorInvalidValue;
  if (p.narrow && a.nq > NB) return hipErrorInvalidValue;
  if (a.mask && ((uintptr_t)a.mask & 7)) return hipErrorInvalidValue;
  if (a.join && ((long)a.q_off + a.nq > a.N || a.col0 != ((unsigned)a.q_off & ~63u))) return hipErrorInvalidValue;
  if (!a.join && a.col0 != 0) return hipErrorInvalidValue;
  if (a.capacity < 1 || a.capacity > kRangeMaxRecords) return hipErrorInvalidValue;
  if (!a.q || !a.g || !a.out_query || !a.out_row || !a.out_score || !a.total || ((uintptr_t)a.total & 7))
    return hipErrorInvalidValue;
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  kRange[a.dtype][a.mask != nullptr](a);
  return hipGetLastError();
}

}  // namespace clipgpu
