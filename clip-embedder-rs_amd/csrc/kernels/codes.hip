// Int8 codes of the embedding index and the coarse scan over them (clipgpu_index_enable_codes,
// clipgpu_index_search_coded): a compressed copy of the gallery that is scanned with
// v_mfma_i32_16x16x64_i8, the first stage of a search whose second stage re-ranks a short candidate list
// per query exactly (kernels/probe.hip on the candidates as lists).
//
// Codes (codes_quant_kernel).  A row x, as stored and widened to f32, becomes int8 [Ep], Ep = E rounded up to
// 64, the bytes past E zero, and one f32 scale; every operation is a single f32 operation:
//
//   m = max |x_i|;  m not finite, m == 0 or 127 / m not finite: codes 0, scale 0;  else
//   inv = 127 / m;  code_i = clamp(rint(x_i * inv), -127, 127) (nearest even);  scale = m / 127
//
// A NaN anywhere in the row is found by its own test (fmaxf would lose it) and makes m non-finite.
//
// Coarse score (codes_scan_kernel).  d = sum_i cq_i * cg_i in int32, exact and independent of the order of
// the sum (|d| <= 1024 * 127^2 < 2^24 for E <= 1024, so f32(d) is exact as well), and
// coarse[q][j] = f32(d) * scale[j], one f32 multiply, negated when the search's logit scale is negative.  The
// query's scale is one positive factor for all of its rows and is left out.  Query q's candidates are the k
// largest topk_key(bits(coarse), j) over the rows the mask allows: the search's key, so the result does not
// depend on spans, routes or the order rows are met in.
//
// The kernel.  A wave owns one 16-row query tile and a gallery span, walked in 16-row tiles.  No operand
// passes through LDS: an integer dot product does not care which k a lane supplies as long as both operands
// agree, so per 64-byte k step lane l loads the 16 bytes at row (l & 15), byte 64 * step + 16 * (l >> 4) of
// the code rows, for A (queries) and B (gallery) alike.  The query fragments are loaded once and stay in
// registers (S steps of four VGPRs); the accumulator has the usual map, col = lane & 15 (gallery row),
// row = (lane >> 4) * 4 + reg (query).  A gallery tile is requested two tiles ahead into one of two register
// sets, every request the same loads whatever the position (the steps past Ep / 64 of an instantiation read
// the last step again and no MFMA uses them), with its rows' scales and, MASKED, its rows' mask words; rows
// past the end of the gallery are clamped for the loads and kept out of the selection.  The two halves of the
// k steps run as two accumulator chains, added at the end: integers, so the sum is the same.
// Selection: the few-query kernel's (kernels/topk.hip), entries (coarse bits, row) in launch_topk_merge's layout.
//
// Two shapes of one kernel: a block of one wave (at most 16 queries: the few-query route of topk_plan), and a
// block of four waves that own four query tiles of the same span and meet its tiles in the cache together
// (the wide route).  The waves of a block share nothing else; there is no block barrier.
#include <cfloat>
#include <cstdint>

#include "common.hpp"
#include "gallery.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_select.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// One wave per row; row j = ids[i] (ids given) or first + i, of src and of the codes alike.
template <typename GT>
__global__ __launch_bounds__(256) void codes_quant_kernel(const GT* __restrict__ src, long n, int E, int Ep,
                                                          const int64_t* __restrict__ ids, long first,
                                                          int8_t* __restrict__ codes, float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // whole waves leave; no block barrier
  const long j = ids ? ids[i] : first + i;
  const GT* x = src + j * E;
  float m = 0.f;
  bool bad = false;  // an inf or a NaN
  for (int c = lane * 4; c < E; c += 256) {
    const float4 v = gal_widen<GT>(gal_raw(x + c));
    const float a[4] = {fabsf(v.x), fabsf(v.y), fabsf(v.z), fabsf(v.w)};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bad = bad || !(a[t] <= FLT_MAX);
      m = fmaxf(m, a[t]);
    }
  }
  m = wave_max(m);
  float inv = 0.f, sc = 0.f;
  bool zero = __ballot(bad) != 0 || m == 0.f;
  if (!zero) {
    inv = __fdiv_rn(127.0f, m);
    zero = !(inv <= FLT_MAX);
    if (!zero) sc = __fdiv_rn(m, 127.0f);
  }
  auto code = [&](float v) { return (uint32_t)max(-127, min(127, __float2int_rn(__fmul_rn(v, inv)))) & 0xffu; };
  uint32_t* dst = (uint32_t*)(codes + j * Ep);
  for (int c = lane * 4; c < Ep; c += 256) {
    uint32_t w = 0;
    if (c < E && !zero) {
      const float4 v = gal_widen<GT>(gal_raw(x + c));
      w = code(v.x) | (code(v.y) << 8) | (code(v.z) << 16) | (code(v.w) << 24);
    }
    dst[c >> 2] = w;
  }
  if (lane == 0) scale[j] = sc;
}

// KC: list capacity the LDS is sized for (k <= KC); S: k steps the registers hold (Ep / 64 <= S); WAVES: query
// tiles per block.  LDS: WAVES * 16 * (KC + 32) entries and nothing else.
template <int KC, int S, int WAVES, bool MASKED>
__global__ __launch_bounds__(64 * WAVES) void codes_scan_kernel(const int8_t* __restrict__ qc,
                                                                const int8_t* __restrict__ gc,
                                                                const float* __restrict__ gscale, int nq, int N, int Ep,
                                                                int neg, int k, int span_cols, int n_spans,
                                                                uint2* __restrict__ ws,
                                                                const uint32_t* __restrict__ mask) {
  constexpr int STRIDE = KC + CAND1;
  static_assert(S % 2 == 0, "the k steps run as two chains");
  __shared__ uint2 sel_all[WAVES][NB * STRIDE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = (blockIdx.x * WAVES + wave) * NB, span = blockIdx.y;
  if (q0 >= nq) return;  // whole waves leave; the kernel has no block barrier
  const int rows = min(NB, nq - q0);
  uint2* sel = sel_all[wave];
  const unsigned c_begin = (unsigned)span * span_cols;  // < N
  const unsigned c_end = min((unsigned)N, c_begin + span_cols);
  if constexpr (MASKED) {  // a span with no allowed row: k empty entries per query row, nothing requested
    unsigned any = 0;
    for (unsigned w = (c_begin >> 5) + lane; w < ((c_end + 63) >> 6) * 2; w += 64) any |= mask[w];
    if (__ballot(any != 0) == 0) {
      for (int row = 0; row < rows; ++row) {
        uint2* dst = ws + ((long)(q0 + row) * n_spans + span) * k;
        for (int t = lane; t < k; t += 64) dst[t] = ent_empty();
      }
      return;
    }
  }
  for (int i = lane; i < NB * STRIDE; i += 64) sel[i] = ent_empty();
  wave_lds_order();
  const int r = lane & 15, qd = lane >> 4;
  const int steps = Ep / 64, last_step = steps - 1;
  const unsigned nmax = (unsigned)N - 1;
  // The thresholds and the candidate counts of rows 4 * qd + e, the same value in the 16 lanes of a row group:
  // in registers (a count in LDS would be the 256 bytes by which two four-wave blocks at KC = 128 miss a CU).
  uint64_t thr[4] = {0, 0, 0, 0};
  int cn[4] = {0, 0, 0, 0};
  i32x4 a[S];  // the query tile: row r, bytes 64 s + 16 qd
  {
    const int8_t* pq = qc + (long)min(q0 + r, nq - 1) * Ep + 16 * qd;
#pragma unroll
    for (int s = 0; s < S; ++s) a[s] = *(const i32x4*)(pq + 64 * min(s, last_step));
  }
  unsigned lj = c_begin;  // the next tile to request
  // One request: the mask word (MASKED), the scale and S code loads of gallery row lj + r -- the same loads
  // whatever the position, so that the loads in flight can be counted.
  auto request = [&](i32x4(&vb)[S], float& vs, uint32_t& vm) {
    const unsigned row = min(lj + r, nmax);
    if constexpr (MASKED) vm = mask[row >> 5];
    vs = gscale[row];
    const int8_t* p = gc + (long)row * Ep + 16 * qd;
#pragma unroll
    for (int s = 0; s < S; ++s) vb[s] = *(const i32x4*)(p + 64 * min(s, last_step));
    lj += NB;
  };
  // C[row = 4 * qd + e][col = r] of the tile at column cj: the few-query kernel's selection on coarse scores.
  auto select = [&](unsigned cj, const i32x4& acc, float sc, bool allowed) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e >= rows) break;  // rows 4 * qd + e >= e: all padding
      const unsigned col = cj + r;
      const int rl = 4 * qd + e;
      const float f = __fmul_rn((float)acc[e], sc);
      const uint32_t bits = __float_as_uint(neg ? -f : f);
      const uint64_t key = topk_key(bits, col);
      const bool live = col < c_end && rl < rows && allowed;
      bool pass = live && key > thr[e];
      uint64_t bal = __ballot(pass);
      if (bal == 0) continue;
      unsigned mq = (unsigned)(bal >> (16 * qd)) & 0xffffu;
      if (__ballot(cn[e] + __popc(mq) > CAND1) != 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // the four rows this ballot covers
          const int c2 = __builtin_amdgcn_readlane(cn[e], 16 * g);
          if (c2 + __popc((unsigned)(bal >> (16 * g)) & 0xffffu) > CAND1) {
            const uint64_t t2 = compact_row(sel + (4 * g + e) * STRIDE, k, c2, lane);
            if (qd == g) {
              thr[e] = t2;
              cn[e] = 0;
            }
          }
        }
        wave_lds_order();
        pass = live && key > thr[e];
        bal = __ballot(pass);
        mq = (unsigned)(bal >> (16 * qd)) & 0xffffu;
      }
      if (pass) sel[rl * STRIDE + k + cn[e] + __popc(mq & ((1u << r) - 1u))] = make_uint2(bits, col);
      wave_lds_order();
      cn[e] += __popc(mq);
    }
  };
  unsigned cj = c_begin;  // the tile in hand
  auto step = [&](i32x4(&vb)[S], float& vs, uint32_t& vm) {
    i32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < S; s += 2) {
      if (s < steps) acc0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], vb[s], acc0, 0, 0, 0);
      if (s + 1 < steps) acc1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s + 1], vb[s + 1], acc1, 0, 0, 0);
    }
    const i32x4 acc = acc0 + acc1;
    const float sc = vs;
    bool allowed = true;
    if constexpr (MASKED) allowed = ((vm >> ((cj + r) & 31)) & 1u) != 0;
    request(vb, vs, vm);  // two tiles ahead, into the registers the MFMAs above have read
    select(cj, acc, sc, allowed);
    cj += NB;
  };
  i32x4 b0[S], b1[S];
  float s0 = 0.f, s1 = 0.f;
  uint32_t m0 = 0, m1 = 0;
  // The steps run in pairs, a fixed number of them: an odd count ends in one step past the span, whose rows
  // request() clamped into the gallery and whose columns are all >= c_end, so none passes.
  request(b0, s0, m0);
  __builtin_amdgcn_sched_barrier(0);
  request(b1, s1, m1);
  __builtin_amdgcn_sched_barrier(0);
  const int n_tiles = (int)((c_end - c_begin + NB - 1) / NB);
  for (int it = 0; it < n_tiles; it += 2) {
    step(b0, s0, m0);
    step(b1, s1, m1);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = 4 * g + e;
      const int c2 = __builtin_amdgcn_readlane(cn[e], 16 * g);
      if (row >= rows) continue;
      if (c2 > 0) compact_row(sel + row * STRIDE, k, c2, lane);
      uint2* dst = ws + ((long)(q0 + row) * n_spans + span) * k;
      for (int t = lane; t < k; t += 64) dst[t] = sel[row * STRIDE + t];
    }
}

// One wave per query: its merged candidates (int64, -1 padded behind the valid ones) as the lists the probe
// kernel reads.  List 2q = the candidates of query q, list 2q + 1 = its padding, which nothing probes.
__global__ __launch_bounds__(256) void codes_lists_kernel(const int64_t* __restrict__ cand, int nq, int refine,
                                                          int32_t* __restrict__ ids, int32_t* __restrict__ offsets,
                                                          int64_t* __restrict__ lists) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  int valid = 0;
  for (int base = 0; base < refine; base += 64) {
    const int t = base + lane;
    const int64_t v = t < refine ? cand[(long)q * refine + t] : -1;
    if (t < refine) ids[(long)q * refine + t] = v < 0 ? 0 : (int32_t)v;
    valid += __popcll(__ballot(v >= 0));
  }
  if (lane == 0) {
    offsets[2 * q] = q * refine;
    offsets[2 * q + 1] = q * refine + valid;
    if (q == nq - 1) offsets[2 * nq] = nq * refine;
    lists[q] = 2 * q;
  }
}

template <int KC, int S, int WAVES, bool MASKED>
void launch_scan_one(const CodesScanArgs& a) {
  const TopkPlan& p = a.plan;
  hipLaunchKernelGGL((codes_scan_kernel<KC, S, WAVES, MASKED>), dim3((a.nq + NB * WAVES - 1) / (NB * WAVES), p.n_spans),
                     dim3(64 * WAVES), 0, a.stream, a.qc, a.gc, a.gscale, a.nq, a.N, a.Ep, a.neg ? 1 : 0, a.k, p.span_cols,
                     p.n_spans, (uint2*)a.ws, a.mask);
}

// Every instantiation: [k steps 2 / 8 / 16][four waves][MASKED][list capacity 16 / 32 / 64 / 128].
typedef void (*Scan)(const CodesScanArgs&);
#define SCAN_KC(S, W, M) \
  { launch_scan_one<16, S, W, M>, launch_scan_one<32, S, W, M>, launch_scan_one<64, S, W, M>, launch_scan_one<128, S, W, M> }
#define SCAN_S(S) \
  { {SCAN_KC(S, 1, false), SCAN_KC(S, 1, true)}, {SCAN_KC(S, 4, false), SCAN_KC(S, 4, true)} }
constexpr Scan kScan[3][2][2][4] = {SCAN_S(2), SCAN_S(8), SCAN_S(16)};

}  // namespace

hipError_t launch_codes_quant(const CodesQuantArgs& a) {
  if (!a.src || !a.codes || !a.scale || a.n <= 0 || a.E <= 0 || a.E % 16 != 0 || a.Ep < a.E || a.Ep % 64 != 0)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.n + 3) / 4));
  if (a.dtype == TOPK_GAL_F32)
    hipLaunchKernelGGL(codes_quant_kernel<float>, grid, dim3(256), 0, a.stream, (const float*)a.src, a.n, a.E, a.Ep, a.ids,
                       a.first, a.codes, a.scale);
  else if (a.dtype == TOPK_GAL_F16)
    hipLaunchKernelGGL(codes_quant_kernel<_Float16>, grid, dim3(256), 0, a.stream, (const _Float16*)a.src, a.n, a.E, a.Ep,
                       a.ids, a.first, a.codes, a.scale);
  else if (a.dtype == TOPK_GAL_BF16)
    hipLaunchKernelGGL(codes_quant_kernel<__bf16>, grid, dim3(256), 0, a.stream, (const __bf16*)a.src, a.n, a.E, a.Ep,
                       a.ids, a.first, a.codes, a.scale);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_codes_scan(const CodesScanArgs& a) {
  const TopkPlan& p = a.plan;
  if (!a.qc || !a.gc || !a.gscale || !a.ws || a.nq <= 0 || a.N <= 0 || a.k < 1 || a.k > kTopkMax)
    return hipErrorInvalidValue;
  if (a.Ep <= 0 || a.Ep % 64 != 0 || a.Ep > kCodesMaxE) return hipErrorInvalidValue;
  if (p.span_cols <= 0 || p.span_cols % TB != 0 || (long)p.n_spans * p.span_cols < a.N ||
      (long)(p.n_spans - 1) * p.span_cols >= a.N || (long)p.n_spans * a.k > INT32_MAX || p.n_spans > 65535)
    return hipErrorInvalidValue;
  if (p.narrow && a.nq > NB) return hipErrorInvalidValue;
  if (a.mask && ((uintptr_t)a.mask & 7)) return hipErrorInvalidValue;
  const int si = a.Ep <= 128 ? 0 : a.Ep <= 512 ? 1 : 2;
  const int kc = a.k <= 16 ? 0 : a.k <= 32 ? 1 : a.k <= 64 ? 2 : 3;
  kScan[si][p.narrow ? 0 : 1][a.mask != nullptr][kc](a);
  return hipGetLastError();
}

hipError_t launch_codes_lists(const int64_t* cand, int nq, int refine, int32_t* ids, int32_t* offsets, int64_t* lists,
                              hipStream_t s) {
  if (!cand || !ids || !offsets || !lists || nq <= 0 || refine < 1 || refine > kTopkMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(codes_lists_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, cand, nq, refine, ids, offsets, lists);
  return hipGetLastError();
}

}  // namespace clipgpu
