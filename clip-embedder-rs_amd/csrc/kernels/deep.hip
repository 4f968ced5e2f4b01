// Deep top-k search of a device-resident gallery (clipgpu_index_search_deep): the first k rows of the search's
// order for 1 <= k <= kDeepKMax = 4096, without a k-deep list per (query row, span) and without the [n_q][N]
// score matrix.
//
//   key(i, j) = topk_key(bits of fmaf(dot(q[i], g[j]), scale, bias), j)      unique per (i, j), topk_key.hpp
//
// The k-th largest key of a query is found by a radix select, 8 bits per pass from the top, at most 8 passes;
// then every key at or above it is emitted and the candidates are sorted.  Per query of a chunk (at most 256)
// the device keeps the key bits fixed so far (prefix), the count of keys strictly above the prefix's bucket
// (above) and a done flag.
//
//   histogram pass p   deep_wide_kernel / deep_narrow_kernel<HIST>: range.hip's two loops (the 64-query tile
//     against gallery spans; the one-wave 16-row tile), the same v_mfma_f32_16x16x4_f32 chain in the same k
//     order through topk_stage.hpp, so every pass sees the search's score bits.  Epilogue: every in-range,
//     live, allowed column whose key has the query's first p digits adds one to hist[query][digit p] in LDS.
//     The lanes of a wave that hit the same bin are counted by ballots and make one LDS add (in pass 0 nearly
//     every score of a row shares the sign-and-exponent bin).  At the end of the span the block adds its
//     non-zero bins to the global histograms with vector atomics.  A block whose queries are all done
//     returns at once.  LDS: 64 x 256 x 4 B = 64 KiB of bins beside the 44 KiB staging, one block per CU
//     (few-query: 16 KiB + 11 KiB).
//   decide             deep_decide_kernel, one wave per query: from the top, the bin b at which above +
//     suffix first reaches k becomes digit p; the bins above b go to `above`; the bins are cleared.  done when
//     above + count(b) <= cand (the candidate capacity, >= k), or when all keys together are fewer than k
//     (pass 0 only: everything is a candidate, the prefix stays 0).  After 8 digits a bin is one key: done.
//   emit               the same two loops<EMIT>: a column is a candidate if key >= prefix (zeros below the
//     fixed digits); a wave ballot of "any candidate" is zero for nearly every tile; a candidate takes a slot
//     from its query's own counter and writes (key, score bits) -- -0 and +0 share a key, so the bits travel.
//   sort               deep_sort_kernel, one block per query: keys and 16-bit record positions in LDS
//     (8192 x 10 B = 80 KiB), a bitonic sort descending by key, the first k out as (int64 row, f32 score),
//     the rest (-1, -inf).
//
// launch_deep enqueues init, 8 x (histogram, decide), emit, sort for one chunk and reads nothing back.
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

std::atomic<int> g_deep_cand{0};

namespace {

enum DeepMode { DEEP_HIST = 0, DEEP_EMIT = 1 };
constexpr int kBins = 256;
// A query's slot counter has a 128-byte line to itself: the emit pass's atomics of different queries do not
// queue behind one another.
constexpr int kCountStride = 32;

// Wave-cooperative (all 64 lanes, uniform control flow): every lane with `valid` adds one to hist[addr]; the
// lanes that share an address make one LDS add between them.  The 16 lanes of a group hold one query row
// (addr = row * 256 + digit).  First, in every group at once: the valid lanes that share the bin of the group's
// first valid lane are counted by one ballot and added by that lane -- in pass 0 that is nearly every lane.
// Then the lanes left over, one distinct address per round.
__device__ __forceinline__ void hist_add(unsigned* hist, bool valid, unsigned addr, int lane) {
  const uint64_t group = 0xffffull << (lane & 48);
  const uint64_t gv = __ballot(valid) & group;
  const int first = gv ? __ffsll((unsigned long long)gv) - 1 : lane;
  const bool same = valid && addr == (unsigned)__shfl((int)addr, first);
  const uint64_t gs = __ballot(same) & group;
  if (gv != 0 && lane == first) atomicAdd(&hist[addr], (unsigned)__popcll(gs));
  valid = valid && !same;
  uint64_t pend = __ballot(valid);
  while (pend) {
    const int lead_lane = __ffsll((unsigned long long)pend) - 1;
    const unsigned lead = (unsigned)__builtin_amdgcn_readlane((int)addr, lead_lane);
    const uint64_t match = __ballot(valid && addr == lead);
    if (lane == lead_lane) atomicAdd(&hist[lead], (unsigned)__popcll(match));
    pend &= ~match;
  }
}

// Does the key carry the first `pass` digits of the prefix?  shift = 56 - 8 * pass, the next digit's position.
__device__ __forceinline__ bool has_prefix(unsigned long long key, unsigned long long prefix, int pass, int shift) {
  return pass == 0 || ((key ^ prefix) >> (shift + 8)) == 0;
}

// One candidate of chunk row `row`: a slot from the row's counter, the record if the slot is inside.
__device__ __forceinline__ void put_candidate(const DeepWork& w, unsigned cand, int row, unsigned long long key,
                                              uint32_t bits) {
  const unsigned pos = atomicAdd(&w.count[row * kCountStride], 1u);
  if (pos < cand) {
    w.rec_key[(size_t)row * cand + pos] = key;
    w.rec_bits[(size_t)row * cand + pos] = bits;
  }
}

// Block: 64 queries x one gallery span, as range_wide_kernel.  HIST: 108 KiB of LDS, one block per CU; EMIT:
// 44 KiB, three.
template <typename GT, bool MASKED, int MODE>
__global__ __launch_bounds__(256, MODE == DEEP_EMIT ? 3 : 1) void deep_wide_kernel(
    const float* __restrict__ qry, const GT* __restrict__ gal, int nq, int N, int E, float scale, float bias,
    int span_cols, const uint2* __restrict__ mask, int pass, unsigned cand, DeepWork w) {
  __shared__ __attribute__((aligned(16))) float stage[2][TB * LDT];  // A | B: [row][k slot qd][k step]
  __shared__ unsigned hist[MODE == DEEP_HIST ? TB * kBins : 1];      // [query row of the tile][digit]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * TB, span = blockIdx.y;
  const int shift = 56 - 8 * pass;
  if constexpr (MODE == DEEP_HIST) {  // every query of the tile is done (block-uniform): nothing to count
    const bool idle = tid >= TB || i0 + tid >= nq || w.done[i0 + tid] != 0;
    if (__syncthreads_and((int)idle)) return;
  }
  // columns as unsigned: N < 2^31, but the last tile's padding columns may reach 2^31
  const unsigned c_begin = (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {  // a span with no allowed row (block-uniform): nothing to do
    unsigned any = 0;
    for (unsigned t = (c_begin >> 6) + tid; t < ((c_end + 63) >> 6); t += 256) any |= mask[t].x | mask[t].y;
    if (!__syncthreads_or((int)(any != 0))) return;
  }
  if constexpr (MODE == DEEP_HIST) {
    for (int i = tid; i < TB * kBins; i += 256) hist[i] = 0;
    __syncthreads();
  }
  const int rowbase = wave * 16;
  const int r = lane & 15, qd = lane >> 4;
  // rows rowbase + 4 * qd + e: whether they take part (inside the chunk; HIST: not done) and their prefixes
  bool rowok[4];
  unsigned long long pre[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = i0 + rowbase + 4 * qd + e;
    rowok[e] = row < nq;
    pre[e] = rowok[e] ? w.prefix[row] : 0ull;
    if constexpr (MODE == DEEP_HIST)
      if (rowok[e]) rowok[e] = w.done[row] == 0;
  }
  // Staging: as range_wide_kernel (thread -> rows tid / 16 + 16 p, k step tid % 16; the next slab's loads are
  // issued before this slab's MFMAs).
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
    auto key_of = [&](int e, int t, uint32_t& bits, bool& ok) {
      const unsigned col = j0 + t * 16 + r;
      ok = col < c_end && rowok[e];
      if constexpr (MASKED) ok = ok && (((t < 2 ? mw.x : mw.y) >> ((t & 1) * 16 + r)) & 1u) != 0;
      bits = __float_as_uint(fmaf(acc[t][e], scale, bias));
      return (unsigned long long)topk_key(bits, col);
    };
    if constexpr (MODE == DEEP_HIST) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          uint32_t bits;
          bool ok;
          const unsigned long long key = key_of(e, t, bits, ok);
          ok = ok && has_prefix(key, pre[e], pass, shift);
          hist_add(hist, ok, (unsigned)(rowbase + 4 * qd + e) * kBins + (unsigned)((key >> shift) & 255u), lane);
        }
    } else {
      unsigned hit = 0;  // bit 4 * e + t
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          uint32_t bits;
          bool ok;
          const unsigned long long key = key_of(e, t, bits, ok);
          if (ok && key >= pre[e]) hit |= 1u << (4 * e + t);
        }
      if (__ballot(hit != 0) == 0) continue;  // wave-uniform: the common case
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if ((hit >> (4 * e + t)) & 1u) {
            uint32_t bits;
            bool ok;
            const unsigned long long key = key_of(e, t, bits, ok);
            put_candidate(w, cand, i0 + rowbase + 4 * qd + e, key, bits);
          }
    }
  }
  if constexpr (MODE == DEEP_HIST) {
    __syncthreads();
    for (int i = tid; i < TB * kBins; i += 256) {
      const unsigned v = hist[i];
      const int row = i0 + (i >> 8);
      if (v != 0 && row < nq) atomicAdd(&w.hist[row * kBins + (i & 255)], v);
    }
  }
}

// One wave: a 16-row query tile against a gallery span in 16-column tiles, as range_narrow_kernel (the same
// flat sequence of requests two slabs ahead, no block barrier).  HIST: 16 KiB of bins beside the 11 KiB.
template <typename GT, bool MASKED, int MODE>
__global__ __launch_bounds__(64) void deep_narrow_kernel(const float* __restrict__ qry, const GT* __restrict__ gal,
                                                         int nq, int N, int E, float scale, float bias, int span_cols,
                                                         const uint32_t* __restrict__ mask, int pass, unsigned cand,
                                                         DeepWork w) {
  typedef typename GalRaw<GT>::type raw_t;
  __shared__ __attribute__((aligned(16))) float stage[2][NB * LDT];  // A | B: [row][k slot qd][k step]
  __shared__ unsigned hist[MODE == DEEP_HIST ? NB * kBins : 1];      // [query row][digit]
  const int lane = threadIdx.x, span = blockIdx.x;
  const int shift = 56 - 8 * pass;
  if constexpr (MODE == DEEP_HIST) {  // every query is done: nothing to count
    const bool idle = lane >= nq || w.done[min(lane, nq - 1)] != 0;
    if (__ballot(!idle) == 0) return;
  }
  const unsigned c_begin = (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {  // a span with no allowed row: nothing requested
    unsigned any = 0;
    for (unsigned t = (c_begin >> 5) + lane; t < ((c_end + 63) >> 6) * 2; t += 64) any |= mask[t];
    if (__ballot(any != 0) == 0) return;
  }
  if constexpr (MODE == DEEP_HIST) {
    for (int i = lane; i < NB * kBins; i += 64) hist[i] = 0;
    wave_lds_order();
  }
  const int r = lane & 15, qd = lane >> 4;
  bool rowok[4];  // rows 4 * qd + e, as in the wide kernel
  unsigned long long pre[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = 4 * qd + e;
    rowok[e] = row < nq;
    pre[e] = rowok[e] ? w.prefix[row] : 0ull;
    if constexpr (MODE == DEEP_HIST)
      if (rowok[e]) rowok[e] = w.done[row] == 0;
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
  // C[row = 4 * qd + e][col = r] of the tile at column cj
  auto tail = [&](unsigned cj, const f32x4& acc, bool allowed) {
    const unsigned col = cj + r;
    const bool colok = col < c_end && allowed;
    if constexpr (MODE == DEEP_HIST) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned long long key = topk_key(__float_as_uint(fmaf(acc[e], scale, bias)), col);
        const bool ok = colok && rowok[e] && has_prefix(key, pre[e], pass, shift);
        hist_add(hist, ok, (unsigned)(4 * qd + e) * kBins + (unsigned)((key >> shift) & 255u), lane);
      }
    } else {
      unsigned hit = 0;  // bit e
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (colok && rowok[e] && topk_key(__float_as_uint(fmaf(acc[e], scale, bias)), col) >= pre[e]) hit |= 1u << e;
      if (__ballot(hit != 0) == 0) return;  // wave-uniform: the common case
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((hit >> e) & 1u) {
          const uint32_t bits = __float_as_uint(fmaf(acc[e], scale, bias));
          put_candidate(w, cand, 4 * qd + e, topk_key(bits, col), bits);
        }
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
    // the bit of column cj + r, taken before the request reuses the word's register (range_narrow_kernel)
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
      tail(cj, acc, allowed);
      acc = f32x4{0.f, 0.f, 0.f, 0.f};
      ck = 0;
      cj += NB;
    }
  };
  float4 a0[4] = {}, a1[4] = {};
  raw_t b0[4] = {}, b1[4] = {};
  uint32_t m0 = 0, m1 = 0;
  // An odd count of steps ends in one step past the span: it stages rows that request() clamped into the
  // gallery, and if it completes a tile, every column of it is >= c_end and none counts.
  request(a0, b0, m0);
  __builtin_amdgcn_sched_barrier(0);
  request(a1, b1, m1);
  __builtin_amdgcn_sched_barrier(0);
  const int n_steps = (int)((c_end - c_begin + NB - 1) / NB) * ((E + TK - 1) / TK);
  for (int it = 0; it < n_steps; it += 2) {
    step(a0, b0, m0);
    step(a1, b1, m1);
  }
  if constexpr (MODE == DEEP_HIST) {
    wave_lds_order();
    for (int i = lane; i < NB * kBins; i += 64) {
      const unsigned v = hist[i];
      if (v != 0 && (i >> 8) < nq) atomicAdd(&w.hist[i], v);
    }
  }
}

// A chunk's state before its first pass: bins, prefixes, counts and flags zero.  Grid kDeepChunk blocks of 256.
__global__ __launch_bounds__(256) void deep_init_kernel(DeepWork w) {
  const int b = blockIdx.x, t = threadIdx.x;
  w.hist[b * kBins + t] = 0;
  if (b == 0) {
    w.prefix[t] = 0ull;
    w.above[t] = 0;
    w.done[t] = 0;
    w.count[t * kCountStride] = 0;
    w.passes[t] = 0;
  }
}

// One wave per query: digit `pass` of the k-th key from the query's bins (lane l holds bins 4 l .. 4 l + 3).
__global__ __launch_bounds__(64) void deep_decide_kernel(unsigned k, unsigned cand, int pass, DeepWork w) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (w.done[q] != 0) return;  // its bins were not touched
  uint4* bins = (uint4*)(w.hist + q * kBins) + lane;
  const uint4 c = *bins;
  *bins = make_uint4(0, 0, 0, 0);
  const unsigned s = c.x + c.y + c.z + c.w;
  unsigned inc = s;  // the bins of lanes >= this one
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_down(inc, d);
    if (lane + d < 64) inc += o;
  }
  unsigned run = w.above[q] + (inc - s);  // the keys above this lane's bins
  const unsigned cs[4] = {c.x, c.y, c.z, c.w};
  int b = -1;
  unsigned ab = 0, cb = 0;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    if (b < 0 && run + cs[j] >= k) {
      b = 4 * lane + j;
      ab = run;
      cb = cs[j];
    }
    run += cs[j];
  }
  const uint64_t found = __ballot(b >= 0);  // the lanes at and below the one that holds the bin
  if (found == 0) {                         // fewer keys than k: all of them are candidates
    if (lane == 0) {
      w.done[q] = 1;
      w.passes[q] = pass + 1;
    }
    return;
  }
  if (lane == 63 - __clzll((unsigned long long)found)) {
    w.prefix[q] |= (unsigned long long)b << (56 - 8 * pass);
    w.above[q] = ab;
    w.passes[q] = pass + 1;
    if (ab + cb <= cand) w.done[q] = 1;
  }
}

// One block per query: its candidates sorted descending by key, the first k written out.
constexpr int kSortThreads = 1024;
__global__ __launch_bounds__(kSortThreads) void deep_sort_kernel(int k, unsigned cand, DeepWork w, int64_t* out_idx,
                                                                 float* out_score, int32_t* out_passes) {
  __shared__ unsigned long long keys[kDeepCandMax];
  __shared__ unsigned short where[kDeepCandMax];  // the record a key came from
  const int q = blockIdx.x, tid = threadIdx.x;
  const unsigned n = min(w.count[q * kCountStride], cand);
  unsigned P = 2;
  while (P < n) P <<= 1;  // <= kDeepCandMax
  for (unsigned i = tid; i < P; i += kSortThreads) {
    keys[i] = i < n ? w.rec_key[(size_t)q * cand + i] : 0ull;  // key 0: the empty slot, below every key
    where[i] = (unsigned short)i;
  }
  for (unsigned size = 2; size <= P; size <<= 1)
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (unsigned t = tid; t < P / 2; t += kSortThreads) {
        const unsigned i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride;
        const unsigned long long a = keys[i], b = keys[j];
        if ((a < b) == ((i & size) == 0)) {  // descending where bit `size` of i is clear
          keys[i] = b;
          keys[j] = a;
          const unsigned short x = where[i];
          where[i] = where[j];
          where[j] = x;
        }
      }
    }
  __syncthreads();
  for (unsigned s = tid; s < (unsigned)k; s += kSortThreads) {
    const bool have = s < n;
    out_idx[(size_t)q * k + s] = have ? (int64_t)(uint32_t)~(uint32_t)keys[s] : -1;
    out_score[(size_t)q * k + s] = have ? __uint_as_float(w.rec_bits[(size_t)q * cand + where[s]]) : -INFINITY;
  }
  if (out_passes && tid == 0) out_passes[q] = w.passes[q];
}

template <typename GT, bool MASKED, int MODE>
void launch_deep_scan(const DeepArgs& a, int pass, unsigned cand) {
  const TopkPlan& p = a.plan;
  if (p.narrow)
    hipLaunchKernelGGL((deep_narrow_kernel<GT, MASKED, MODE>), dim3(p.n_spans), dim3(64), 0, a.stream, a.q,
                       (const GT*)a.g, a.nq, a.N, a.E, a.scale, a.bias, p.span_cols, a.mask, pass, cand, a.work);
  else
    hipLaunchKernelGGL((deep_wide_kernel<GT, MASKED, MODE>), dim3((a.nq + TB - 1) / TB, p.n_spans), dim3(256), 0,
                       a.stream, a.q, (const GT*)a.g, a.nq, a.N, a.E, a.scale, a.bias, p.span_cols,
                       (const uint2*)a.mask, pass, cand, a.work);
}

// Every instantiation: [gallery type][MASKED][mode].
typedef void (*DeepScan)(const DeepArgs&, int, unsigned);
#define DEEP_M(GT, M) { launch_deep_scan<GT, M, DEEP_HIST>, launch_deep_scan<GT, M, DEEP_EMIT> }
#define DEEP_GT(GT) { DEEP_M(GT, false), DEEP_M(GT, true) }
constexpr DeepScan kDeepScan[3][2][2] = {DEEP_GT(float), DEEP_GT(_Float16), DEEP_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kDeepScan");

}  // namespace

int deep_cand(int k) {
  const int n = g_deep_cand.load();
  return std::max(k, n > 0 ? n : kDeepCandMax);
}

size_t deep_carve(char* base, DeepWork* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~size_t(255);
    return p;
  };
  w->hist = (unsigned*)take((size_t)kDeepChunk * kBins * 4);
  w->prefix = (unsigned long long*)take((size_t)kDeepChunk * 8);
  w->above = (unsigned*)take((size_t)kDeepChunk * 4);
  w->done = (int*)take((size_t)kDeepChunk * 4);
  w->count = (unsigned*)take((size_t)kDeepChunk * kCountStride * 4);
  w->passes = (int*)take((size_t)kDeepChunk * 4);
  w->rec_key = (unsigned long long*)take((size_t)kDeepChunk * kDeepCandMax * 8);
  w->rec_bits = (unsigned*)take((size_t)kDeepChunk * kDeepCandMax * 4);
  return off;
}

hipError_t launch_deep(const DeepArgs& a) {
  const TopkPlan& p = a.plan;
  if (a.nq <= 0 || a.nq > kDeepChunk || a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.k < 1 || a.k > kDeepKMax)
    return hipErrorInvalidValue;
  if (p.span_cols <= 0 || p.span_cols % TB != 0 || (long)p.n_spans * p.span_cols < a.N ||
      (long)(p.n_spans - 1) * p.span_cols >= a.N || p.n_spans > 65535)
    return hipErrorInvalidValue;
  if (p.narrow && a.nq > NB) return hipErrorInvalidValue;
  if (a.mask && ((uintptr_t)a.mask & 7)) return hipErrorInvalidValue;
  if (!a.q || !a.g || !a.out_idx || !a.out_score || !a.work.hist || !a.work.rec_key) return hipErrorInvalidValue;
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  const unsigned cand = (unsigned)deep_cand(a.k);  // kDeepCandMax at most: the records and the sort's LDS hold it
  if (cand > (unsigned)kDeepCandMax) return hipErrorInvalidValue;
  const DeepScan* scan = kDeepScan[a.dtype][a.mask != nullptr];
  hipLaunchKernelGGL(deep_init_kernel, dim3(kDeepChunk), dim3(256), 0, a.stream, a.work);
  for (int pass = 0; pass < 8; ++pass) {
    scan[DEEP_HIST](a, pass, cand);
    hipLaunchKernelGGL(deep_decide_kernel, dim3(a.nq), dim3(64), 0, a.stream, (unsigned)a.k, cand, pass, a.work);
  }
  scan[DEEP_EMIT](a, 8, cand);
  hipLaunchKernelGGL(deep_sort_kernel, dim3(a.nq), dim3(kSortThreads), 0, a.stream, a.k, cand, a.work, a.out_idx,
                     a.out_score, a.out_passes);
  return hipGetLastError();
}

}  // namespace clipgpu
