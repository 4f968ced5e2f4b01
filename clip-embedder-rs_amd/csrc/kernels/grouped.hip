// Grouped search of the embedding index (clipgpu_index_search_grouped): every gallery row carries a group label,
// and the result is the k best GROUPS, each by its best row -- field collapsing, group-by search.  Neither the
// [queries][N] matrix nor a deep list that one long group could fill is built.
//
//   order          = the search's: descending score, equal scores by ascending row      (topk_key.hpp)
//   representative = a group's first live allowed row in that order
//   result         = the first k representatives, with the search's score bits
//
// Labels: one uint32 per slot.  A caller's label is below 2^31; slot j without one holds 0x80000000 | j, a group
// of its own that collides with nothing (group_fill_kernel, group_set_kernel below).
//
// Phase 1 (topk_grouped_kernel).  Block: ONE wave, a 16-row query tile x a gallery span walked in 16-column
// tiles -- the few-query kernel's shape (kernels/topk.hip) on the grid of kernels/compound.hip: the
// v_mfma_f32_16x16x4_f32 chain through the [k slot][k step] staging of topk_stage.hpp in the same k order, so a
// score has similarity's bits; slabs of 64 k requested two ahead in one flat sequence over (tile, slab), every
// request the same loads.  After the chain lane (r, qd) holds C[4 qd + e][col r], e < 4.  New here:
//
//   1. The label of column lj + r rides with every request, as the mask word does: one more vector load, the same
//      at every position, taken out of its register before the next request is issued.
//   2. COLLAPSE: runs of equal adjacent labels are collapsed in registers before the selection sees them.  The 16
//      columns of a tile are the 16 lanes of one DPP row.  From the labels alone, once per tile: the head and tail
//      flags of the runs and the gate words of a Hillis-Steele segmented scan (row_shr / row_shl 1, 2, 4).  Per e:
//      w = topk_mono(score) + 1 for a column that takes part (in range, live, allowed, a real query row), else 0;
//      an exclusive segmented max-scan of w forward and one backward; the column stays a candidate unless a
//      column of its run to its left has w >= its own or one to its right has w > its own -- the comparison of
//      the 64-bit keys, whose low word favours the lower column.  topk_mono is at most 0xff800000, so w does not
//      wrap; a NaN (mono 0) has w = 1 and the scan's identity 0 belongs to the columns that take no part, which
//      therefore neither survive nor suppress.  Runs that straddle a tile or a span are left to 3.
//   3. The list of a row holds ONE entry per group: grouped_compact_row is a kill pass -- every entry for which
//      another entry of the same label has a larger key becomes empty; keys are unique, so one entry per label
//      survives -- followed by compact_row (topk_select.hpp, untouched).  The threshold it returns is the key of
//      the k-th distinct group's representative so far, 0 while fewer than k groups are known: a column below it
//      cannot be among the first k representatives, whatever its group.  An entry's label is re-read from global
//      memory (labels[entry.y], an L2 hit on the rare path) and broadcast by v_readlane; a parallel LDS array
//      would have cost resident waves (the table in compound.hip) and was not built, so the two were not timed
//      against each other.
//
// Per-span lists of k suffice: let R be a global top-k representative in span s.  An entry of span s that
// outranks R is the span-local best of another group, whose global best then outranks R too; there are fewer than
// k such groups.
//
// Phase 2 (topk_grouped_merge_kernel): topk_merge_kernel's loop (one wave per query row, 64-entry steps) with
// grouped_compact_row, and one more output: the label of each result as int64, -1 for an ungrouped row or an
// empty slot.
//
// LDS per phase-1 block: 11,264 bytes of staging + 16 (KC + 32) 8 of selection state + 64 of counters: the G = 1
// column of the table in compound.hip (KC 16 / 32 / 64 / 128: 17,472 / 19,520 / 23,616 / 31,808 bytes, 9 / 8 / 6 /
// 5 waves per CU); every KC of the few-query kernel is kept, because each adds a wave over the next.
// Vector registers as compiled, the 8 AGPRs included (.vgpr_count of the code object), over KC 16 .. 128:
//                      COLLAPSE off, unmasked / MASKED     COLLAPSE on, unmasked / MASKED
//     f32 gallery           144 .. 148 / 148                    152 / 156
//     16-bit gallery        128 .. 132 / 132                    136 / 140
// 86 .. 100 SGPRs.  No instantiation spills a vector or a scalar register and none uses scratch.  Every one fits 3
// waves per SIMD (12 per CU), above what the LDS admits, so the LDS figure stands.
// The merge: 53 VGPRs, 192 entries of selection state per wave (6,144 bytes per block of 4 waves).
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

std::atomic<int> g_grouped_collapse{0};

namespace {

constexpr int CAND2 = 64;                      // phase 2 (one ballot adds at most 64)
constexpr int MERGE_STEPS = 4;                 // 64-entry steps the merge loads at once (topk.hip has the reason)
constexpr uint32_t kUngrouped = 0x80000000u;   // | slot: the label of a row without one
constexpr uint32_t kNoLabel = 0xffffffffu;     // of an empty entry: no slot has it (capacity < 2^31)

// Lane i of each 16-lane row reads lane i - D (row_shr) or i + D (row_shl); a lane without a source keeps `old`.
template <int D>
__device__ __forceinline__ uint32_t shr16(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x110 + D, 0xF, 0xF, false);
}
template <int D>
__device__ __forceinline__ uint32_t shl16(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x100 + D, 0xF, 0xF, false);
}

// The run structure of a tile's 16 columns, from their labels, as words that gate a scan step: f[s] is ~0 iff no
// run starts in columns (r - 2^s, r] -- column r - 2^s then lies in r's run, if every column between does, which
// the earlier steps have established -- and b[s] likewise for a run's end in [r, r + 2^s).  Words in vector
// registers, not lane masks: as eight conditions they took the scalar registers past their file.
struct RunFlags { uint32_t f[4], b[4]; };
__device__ __forceinline__ RunFlags run_flags(uint32_t lab) {
  RunFlags u;
  u.f[0] = shr16<1>(~lab, lab) == lab ? ~0u : 0u;  // column 0 of the tile is compared with ~lab: a head
  u.b[0] = shl16<1>(~lab, lab) == lab ? ~0u : 0u;
  u.f[1] = u.f[0] & shr16<1>(0u, u.f[0]);
  u.b[1] = u.b[0] & shl16<1>(0u, u.b[0]);
  u.f[2] = u.f[1] & shr16<2>(0u, u.f[1]);
  u.b[2] = u.b[1] & shl16<2>(0u, u.b[1]);
  u.f[3] = u.f[2] & shr16<4>(0u, u.f[2]);
  u.b[3] = u.b[2] & shl16<4>(0u, u.b[2]);
  return u;
}
// Whether a column with word w (0: takes no part) stays a candidate: no column of its run in this tile has a
// larger key.  Two segmented inclusive max-scans (Hillis-Steele; 0 is the identity), each shifted by one.
__device__ __forceinline__ bool run_keeps(const RunFlags& u, uint32_t w) {
  uint32_t a = w, b = w;
  a = max(a, shr16<1>(0u, a) & u.f[0]);
  b = max(b, shl16<1>(0u, b) & u.b[0]);
  a = max(a, shr16<2>(0u, a) & u.f[1]);
  b = max(b, shl16<2>(0u, b) & u.b[1]);
  a = max(a, shr16<4>(0u, a) & u.f[2]);
  b = max(b, shl16<4>(0u, b) & u.b[2]);
  a = max(a, shr16<8>(0u, a) & u.f[3]);
  b = max(b, shl16<8>(0u, b) & u.b[3]);
  const uint32_t left = shr16<1>(0u, a) & u.f[0];   // the best of the run's columns below this one
  const uint32_t right = shl16<1>(0u, b) & u.b[0];  // and above it
  return w != 0u && left < w && right <= w;
}

// compact_row for lists that hold one entry per group.  Wave-cooperative (all 64 lanes, uniform arguments);
// ent[0 .. k) the row's list, ent[k .. k + c) its candidates, k + c <= 192.  The kill pass: lane l holds entries
// l, l + 64, l + 128 with their labels (labels[y] for y < N; an empty entry has none) and, for every entry j,
// takes j's key and label from the lane that holds them; an entry is emptied if an entry of its label has a
// larger key.  Then compact_row: the k best survivors in ent[0 .. k), best first, and the key of ent[k - 1].
__device__ __forceinline__ uint64_t grouped_compact_row(uint2* ent, int k, int c, int lane,
                                                        const uint32_t* __restrict__ labels, unsigned N) {
  const int m = k + c;
  uint32_t klo[3], khi[3], lab[3];
  bool dead[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int i = lane + 64 * s;
    const uint2 e = i < m ? ent[i] : ent_empty();
    const uint64_t key = ent_key(e);
    klo[s] = (uint32_t)key;
    khi[s] = (uint32_t)(key >> 32);
    lab[s] = e.y < N ? labels[e.y] : kNoLabel;
    dead[s] = false;
  }
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int end = min(m - 64 * t, 64);  // entries 64 t .. 64 t + end are held in slot t
    for (int j = 0; j < end; ++j) {
      const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)lab[t], j);
      const uint64_t kj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)khi[t], j) << 32) |
                          (uint32_t)__builtin_amdgcn_readlane((int)klo[t], j);
#pragma unroll
      for (int s = 0; s < 3; ++s) dead[s] = dead[s] || (lj == lab[s] && kj > (((uint64_t)khi[s] << 32) | klo[s]));
    }
  }
#pragma unroll
  for (int s = 0; s < 3; ++s)
    if (lane + 64 * s < m && dead[s]) ent[lane + 64 * s] = ent_empty();
  wave_lds_order();
  return compact_row(ent, k, c, lane);
}

// KC: list capacity the LDS is sized for (k <= KC).  COLLAPSE: step 2 of the file header.
template <int KC, typename GT, bool MASKED, bool COLLAPSE>
__global__ __launch_bounds__(64) void topk_grouped_kernel(const float* __restrict__ qry, const GT* __restrict__ gal,
                                                          int nq, int N, int E, float scale, float bias, int k,
                                                          int span_cols, int n_spans, uint2* __restrict__ ws,
                                                          const uint32_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ labels) {
  typedef typename GalRaw<GT>::type raw_t;
  constexpr int STRIDE = KC + CAND1;
  __shared__ __attribute__((aligned(16))) float stage[2][NB * LDT];  // A | B: [row][k slot qd][k step]
  __shared__ uint2 sel[NB * STRIDE];
  __shared__ int cnt[NB];
  const int lane = threadIdx.x, tile = blockIdx.x, span = blockIdx.y;
  const int q0 = tile * NB;  // the tile's first query row; q0 < nq
  const unsigned c_begin = (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {  // a span with no allowed row: k empty entries per query, nothing requested
    unsigned any = 0;
    for (unsigned w = (c_begin >> 5) + lane; w < ((c_end + 63) >> 6) * 2; w += 64) any |= mask[w];
    if (__ballot(any != 0) == 0) {
      for (int row = 0; row < NB && q0 + row < nq; ++row) {
        uint2* dst = ws + ((long)(q0 + row) * n_spans + span) * k;
        for (int t = lane; t < k; t += 64) dst[t] = ent_empty();
      }
      return;
    }
  }
  for (int i = lane; i < NB * STRIDE; i += 64) sel[i] = ent_empty();
  if (lane < NB) cnt[lane] = 0;
  wave_lds_order();
  const int r = lane & 15, qd = lane >> 4;
  uint64_t thr[4] = {0, 0, 0, 0};  // thresholds of rows 4 * qd + e
  // Staging as in the few-query kernel: lane -> (rows lane / 16 + 4 p, p < 4; k step lane % 16); query rows past
  // nq are clamped for the loads and never enter the selection.
  const int srow = lane >> 4, sj = lane & 15;
  const float* pa[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pa[p] = qry + (long)min(q0 + p * 4 + srow, nq - 1) * E;
  unsigned lj = c_begin;  // the next slab to request: tile lj, k lk
  int lk = 0;
  // Every request is the same eight loads, the label of column lj + r (clamped into the gallery) and, MASKED, the
  // tile's mask word, whatever the position, so that the compiler can count the loads in flight; topk.hip
  // (request) has the reasons and the clamps.
  auto request = [&](float4(&va)[4], raw_t(&vb)[4], uint32_t& vm, uint32_t& vl) {
    const int ko = min(lk + sj * 4, E - 4);
    if constexpr (MASKED) vm = mask[min(lj + 4 * srow, (unsigned)N - 1) >> 5];
    vl = labels[min(lj + sj, (unsigned)N - 1)];
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
  // C[row = 4 * qd + e][col = r] of the tile at column cj, lab the label of column cj + r: the collapse, then the
  // few-query kernel's selection with grouped_compact_row.
  auto select = [&](unsigned cj, const f32x4& acc, bool allowed, uint32_t lab) {
    const unsigned col = cj + r;
    RunFlags runs;
    if constexpr (COLLAPSE) runs = run_flags(lab);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rl = 4 * qd + e;
      const uint32_t bits = __float_as_uint(fmaf(acc[e], scale, bias));
      const uint32_t mono = topk_mono(bits);
      const uint64_t key = ((uint64_t)mono << 32) | (uint32_t)~col;  // topk_key(bits, col)
      bool live = col < c_end && q0 + rl < nq && allowed;
      if constexpr (COLLAPSE) live = run_keeps(runs, live ? mono + 1u : 0u);
      bool pass = live && key > thr[e];
      uint64_t bal = __ballot(pass);
      if (bal == 0) continue;  // wave-uniform: the common case once the thresholds have warmed up
      unsigned mq = (unsigned)(bal >> (16 * qd)) & 0xffffu;
      int c = cnt[rl];
      if (__ballot(c + __popc(mq) > CAND1) != 0) {
        for (int g = 0; g < 4; ++g) {  // the four rows this ballot covers
          const int row = 4 * g + e;
          const int c2 = cnt[row];
          if (c2 + __popc((unsigned)(bal >> (16 * g)) & 0xffffu) > CAND1) {
            const uint64_t t2 = grouped_compact_row(sel + row * STRIDE, k, c2, lane, labels, (unsigned)N);
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
      if (pass) sel[rl * STRIDE + k + c + __popc(mq & ((1u << r) - 1u))] = make_uint2(bits, col);
      wave_lds_order();
      if (r == 0 && mq != 0) cnt[rl] = c + __popc(mq);
      wave_lds_order();
    }
  };
  unsigned cj = c_begin;  // the slab in hand: tile cj, k ck
  int ck = 0;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step = [&](float4(&va)[4], raw_t(&vb)[4], uint32_t& vm, uint32_t& vl) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      put(stage[0], p, va[p]);
      put(stage[1], p, gal_widen<GT>(vb[p]));
    }
    // the bit and the label of column cj + r, taken before the request below reuses their registers (topk.hip,
    // step, has the reason and the empty asm's)
    uint32_t mbit = 1;
    if constexpr (MASKED) {
      mbit = (vm >> ((cj & 16) + r)) & 1u;
      asm volatile("" : "+v"(mbit));
    }
    uint32_t lab = vl;
    asm volatile("" : "+v"(lab));
    const bool allowed = mbit != 0;
    wave_lds_order();
    request(va, vb, vm, vl);  // two slabs ahead; the slab after this one is already in flight
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
      select(cj, acc, allowed, lab);
      acc = f32x4{0.f, 0.f, 0.f, 0.f};
      ck = 0;
      cj += NB;
    }
  };
  float4 a0[4] = {}, a1[4] = {};
  raw_t b0[4] = {}, b1[4] = {};
  uint32_t m0 = 0, m1 = 0, l0 = 0, l1 = 0;
  // The steps run in pairs, a fixed number of them (topk.hip has the reasons): an odd count ends in one step past
  // the span, which stages clamped rows and, if it completes a tile, selects nothing (every column >= c_end).
  request(a0, b0, m0, l0);
  __builtin_amdgcn_sched_barrier(0);
  request(a1, b1, m1, l1);
  __builtin_amdgcn_sched_barrier(0);
  const int n_steps = (int)((c_end - c_begin + NB - 1) / NB) * ((E + TK - 1) / TK);
  for (int it = 0; it < n_steps; it += 2) {
    step(a0, b0, m0, l0);
    step(a1, b1, m1, l1);
  }
  for (int row = 0; row < NB && q0 + row < nq; ++row) {
    const int c2 = cnt[row];
    if (c2 > 0) grouped_compact_row(sel + row * STRIDE, k, c2, lane, labels, (unsigned)N);
    uint2* dst = ws + ((long)(q0 + row) * n_spans + span) * k;
    for (int t = lane; t < k; t += 64) dst[t] = sel[row * STRIDE + t];
  }
}

// One wave per query row: the first k representatives of the row's n_spans * k partial results.
__global__ __launch_bounds__(256) void topk_grouped_merge_kernel(const uint2* __restrict__ ws, int nq, int n_spans,
                                                                 int k, const uint32_t* __restrict__ labels, unsigned N,
                                                                 int64_t* __restrict__ out_idx,
                                                                 float* __restrict__ out_score,
                                                                 int64_t* __restrict__ out_group) {
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
  for (long base = 0; base < total; base += 64 * MERGE_STEPS) {
    uint2 e4[MERGE_STEPS];
#pragma unroll
    for (int u = 0; u < MERGE_STEPS; ++u) {
      const long i = base + 64 * u + lane;
      e4[u] = i < total ? src[i] : ent_empty();
    }
#pragma unroll
    for (int u = 0; u < MERGE_STEPS; ++u) {
      const uint2 e = e4[u];
      const uint64_t key = ent_key(e);
      bool pass = key > thr;  // an empty entry (key 0) never passes
      uint64_t bal = __ballot(pass);
      if (bal == 0) continue;
      if (c + __popcll(bal) > CAND2) {
        thr = grouped_compact_row(ent, k, c, lane, labels, N);
        c = 0;
        pass = key > thr;
        bal = __ballot(pass);
      }
      if (pass) ent[k + c + __popcll(bal & ((1ull << lane) - 1ull))] = e;
      wave_lds_order();
      c += __popcll(bal);
    }
  }
  if (c > 0) grouped_compact_row(ent, k, c, lane, labels, N);
  for (int t = lane; t < k; t += 64) {
    const uint2 e = ent[t];
    const bool empty = e.y >= N;
    out_idx[(long)row * k + t] = empty ? -1 : (int64_t)e.y;
    out_score[(long)row * k + t] = empty ? -INFINITY : __uint_as_float(e.x);
    if (out_group) {
      const uint32_t lab = empty ? kUngrouped : labels[e.y];
      out_group[(long)row * k + t] = (lab & kUngrouped) ? -1 : (int64_t)lab;
    }
  }
}

// labels[j] = ungrouped, for j in [first, first + n).
__global__ __launch_bounds__(256) void group_fill_kernel(uint32_t* __restrict__ labels, long first, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    labels[first + i] = kUngrouped | (uint32_t)(first + i);
}

// labels[ids[i]] = groups[i], or ungrouped where groups[i] < 0.  An id outside [0, slots) is skipped.
__global__ __launch_bounds__(256) void group_set_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ groups,
                                                        long n, uint32_t* __restrict__ labels, long slots) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int64_t j = ids[i];
    if (j >= 0 && j < slots) labels[j] = groups[i] < 0 ? (kUngrouped | (uint32_t)j) : (uint32_t)groups[i];
  }
}

template <int KC, typename GT, bool MASKED, bool COLLAPSE>
void launch_grouped_one(const GroupedArgs& a) {
  const TopkPlan& p = a.plan;
  hipLaunchKernelGGL((topk_grouped_kernel<KC, GT, MASKED, COLLAPSE>), dim3((a.nq + NB - 1) / NB, p.n_spans), dim3(64), 0,
                     a.stream, a.q, (const GT*)a.g, a.nq, a.N, a.E, a.scale, a.bias, a.k, p.span_cols, p.n_spans,
                     (uint2*)a.ws, a.mask, a.labels);
}

// Every instantiation: [gallery type][MASKED][COLLAPSE][list capacity 16 / 32 / 64 / 128].
typedef void (*Grouped)(const GroupedArgs&);
#define GROUPED_KC(GT, M, C) \
  { launch_grouped_one<16, GT, M, C>, launch_grouped_one<32, GT, M, C>, launch_grouped_one<64, GT, M, C>, \
    launch_grouped_one<128, GT, M, C> }
#define GROUPED_GT(GT) \
  { {GROUPED_KC(GT, false, false), GROUPED_KC(GT, false, true)}, {GROUPED_KC(GT, true, false), GROUPED_KC(GT, true, true)} }
constexpr Grouped kGrouped[3][2][2][4] = {GROUPED_GT(float), GROUPED_GT(_Float16), GROUPED_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kGrouped");

int blocks_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 4096)); }

}  // namespace

bool grouped_collapse() {
  const int v = g_grouped_collapse.load();
  return v == 0 ? kGroupedCollapseDefault : v == 1;
}

hipError_t launch_group_fill(uint32_t* labels, long first, long n, hipStream_t s) {
  if (!labels || first < 0 || n <= 0 || first + n > (1L << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(group_fill_kernel, dim3(blocks_for(n)), dim3(256), 0, s, labels, first, n);
  return hipGetLastError();
}

hipError_t launch_group_set(const int64_t* ids, const int32_t* groups, long n, uint32_t* labels, long slots,
                            hipStream_t s) {
  if (!ids || !groups || !labels || n <= 0 || slots <= 0 || slots > (1L << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(group_set_kernel, dim3(blocks_for(n)), dim3(256), 0, s, ids, groups, n, labels, slots);
  return hipGetLastError();
}

hipError_t launch_grouped(const GroupedArgs& a) {
  const TopkPlan& p = a.plan;
  if (!a.q || !a.g || !a.ws || !a.labels || !a.out_idx || !a.out_score) return hipErrorInvalidValue;
  if (a.nq <= 0 || a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.k < 1 || a.k > kTopkMax) return hipErrorInvalidValue;
  if (p.span_cols <= 0 || p.span_cols % TB != 0 || (long)p.n_spans * p.span_cols < a.N ||
      (long)(p.n_spans - 1) * p.span_cols >= a.N || (long)p.n_spans * a.k > INT32_MAX || p.n_spans > 65535)
    return hipErrorInvalidValue;
  if (((uintptr_t)a.q & 15) || (a.mask && ((uintptr_t)a.mask & 7))) return hipErrorInvalidValue;
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  const int kc = a.k <= 16 ? 0 : a.k <= 32 ? 1 : a.k <= 64 ? 2 : 3;
  kGrouped[a.dtype][a.mask != nullptr][grouped_collapse()][kc](a);
  hipLaunchKernelGGL(topk_grouped_merge_kernel, dim3((a.nq + 3) / 4), dim3(256), 0, a.stream, (const uint2*)a.ws, a.nq,
                     p.n_spans, a.k, a.labels, (unsigned)a.N, a.out_idx, a.out_score, a.out_group);
  return hipGetLastError();
}

}  // namespace clipgpu
