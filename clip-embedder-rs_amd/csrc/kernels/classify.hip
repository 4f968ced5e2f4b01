// Labelling every stored row (clipgpu_index_classify[_device]): for each gallery row the k best of C label
// embeddings, with their probabilities.
//
//   classify_kernel   assign_kernel's scan (kernels/cluster.hip: a block owns 64 gallery rows on the A side and
//                     walks every 64-label tile with the same v_mfma_f32_16x16x4_f32 chain in the same k order
//                     through the same [k slot][k step] staging, so a score carries the search's bits) with a
//                     k-deep selection, k <= 16, and the softmax normaliser beside it.
//
// Selection.  Output row 4 qd + e of a wave's 16 x 64 tile lives in the 16 lanes of DPP row qd, lane r holding
// the columns j0 + 16 t + r.  That row's list -- its 16 largest keys so far, sorted, best first -- is spread over
// the same 16 lanes: slot r in lane r, so a lane holds four (key, score) entries, one per e, and the whole
// selection state of a block is 12 VGPRs.  There is no LDS list and no candidate buffer:
//   test     a lane's candidate passes if its key is above the row's k-th key, a copy of slot k - 1 that every
//            lane of the row keeps (cut[e]); the k-th key only grows, so a label among the final k always passes;
//   skip     one ballot per 16-column step: if no lane of the wave holds a passing candidate, the step is over.
//            After the first tiles that is the common case;
//   insert   else, per e, while some lane holds one: every DPP row picks its lowest such lane, reads that lane's
//            (key, score) with ds_bpermute, and every slot updates itself from its own entry and its left
//            neighbour's (row_shr:1): above the neighbour -> the neighbour's entry moves in; else above its own
//            -> the candidate moves in; else it stays.  Slot 0's neighbour is the largest key.  A row with no
//            candidate inserts key 0, which moves nothing.  Then cut[e] is read again from slot k - 1.
// Keys are unique per label, so the k best do not depend on the order candidates are met in; slots at and past k
// hold the best of what was inserted and are never written out.
//
// Softmax.  Every column below C feeds its lane's running pair (m, s) of its row e by ms_add, columns ascending:
// column c on lane c % 16.  At the end ms_group16 combines the 16 lanes of the row: the maximum exactly, one
// rescale per lane, a four-level add tree.  That is one span of the probability search (kernels/topk.hip) and
// no merge, so its error bound, DESIGN.md (embedding index, labelling stored rows), is the search's with the
// merge's terms left out.  p = expf(l - M) / S.  Sigmoid: similarity.hip's 1 / (1 + expf(-l)), from the logit.
#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

constexpr float kNegInf = -__builtin_huge_valf();

// The running softmax pair and its combination over a DPP row: topk.hip's ms_add / ms_group16, operation for
// operation (the bound is derived from this order).
__device__ __forceinline__ void ms_add(float& m, float& s, float l) {
  const bool up = l > m;
  const float a = expf(up ? m - l : l - m);  // one exp either way; unused for -inf against -inf (NaN)
  if (up) {
    s = s * a + 1.0f;
    m = l;
  } else if (l != kNegInf) {
    s += a;
  }
}
__device__ __forceinline__ float2 ms_group16(float m, float s) {
  const float M = group16_max(m);
  return make_float2(M, group16_sum(m == M ? s : s * expf(m - M)));
}

// The value of the lane to the left in the DPP row (row_shr:1); lane 0 of a row gets `edge`.
__device__ __forceinline__ uint32_t left_u32(uint32_t v, uint32_t edge) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x111, 0xF, 0xF, false);
}

// One candidate (ck, cs) into a row's sorted list, slot r in lane r: see the head of the file.
__device__ __forceinline__ void list_insert(uint64_t& key, float& score, uint64_t ck, float cs) {
  const uint64_t pk = (uint64_t)left_u32((uint32_t)(key >> 32), ~0u) << 32 | left_u32((uint32_t)key, ~0u);
  const float ps = __uint_as_float(left_u32(__float_as_uint(score), 0u));
  if (ck > pk) {
    key = pk;
    score = ps;
  } else if (ck > key) {
    key = ck;
    score = cs;
  }
}

// Block: 64 gallery rows (A) x every label (B) in tiles of 64, as assign_kernel.  44 KiB of LDS.
template <typename GT, bool MASKED, bool SOFTMAX>
__global__ __launch_bounds__(256, 3) void classify_kernel(const GT* __restrict__ gal, const float* __restrict__ lab,
                                                          int N, int C, int E, int k, float scale, float bias,
                                                          const uint2* __restrict__ mask, int32_t* __restrict__ label,
                                                          float* __restrict__ score, float* __restrict__ prob,
                                                          float* __restrict__ norm) {
  __shared__ __attribute__((aligned(16))) float stage[2][TB * LDT];  // A | B: [row][k slot qd][k step]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // rows as unsigned: N < 2^31, but the last tile's padding rows may reach 2^31
  const unsigned i0 = blockIdx.x * (unsigned)TB;
  uint2 mw = make_uint2(~0u, ~0u);  // the tile's allowed bits: rows i0 .. i0 + 31 | i0 + 32 .. i0 + 63
  if constexpr (MASKED) {
    mw = mask[blockIdx.x];
    if ((mw.x | mw.y) == 0) {  // block-uniform: no allowed row, the empty entry for every row in range
      const int rows = (int)min((unsigned)TB, (unsigned)N - i0);
      for (int i = tid; i < rows * k; i += 256) {
        const long at = (long)i0 * k + i;
        label[at] = -1;
        score[at] = kNegInf;
        prob[at] = 0.f;
      }
      if (SOFTMAX && norm && tid < rows) {
        norm[2 * (long)(i0 + tid)] = kNegInf;
        norm[2 * (long)(i0 + tid) + 1] = 0.f;
      }
      return;
    }
  }
  const int rowbase = wave * 16;
  const int r = lane & 15, qd = lane >> 4;
  // Staging: as assign_kernel (thread -> rows tid / 16 + 16 p, k step tid % 16; the next slab's loads are issued
  // before this slab's MFMAs), with the gallery on the A side.
  const int srow = tid >> 4, sj = tid & 15;
  typedef typename GalRaw<GT>::type raw_t;
  auto loada = [&](raw_t(&v)[4], const GT* const(&src)[4], int k0) {
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = k0 + sj * 4 < E ? gal_raw(src[p] + k0) : raw_t{};  // zero bits widen to 0.f
  };
  auto loadb = [&](float4(&v)[4], const float* const(&src)[4], int k0) {
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
  const GT* pa[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pa[p] = gal + (long)min(i0 + p * 16 + srow, (unsigned)N - 1) * E + sj * 4;
  // rows rowbase + 4 * qd + e: slot r of each row's list, key 0 = nothing yet (topk_key.hpp's empty slot); the
  // row's k-th key; this lane's softmax pair
  uint64_t lkey[4] = {0, 0, 0, 0}, cut[4] = {0, 0, 0, 0};
  float lscore[4] = {kNegInf, kNegInf, kNegInf, kNegInf};
  float m[4] = {kNegInf, kNegInf, kNegInf, kNegInf}, s[4] = {0.f, 0.f, 0.f, 0.f};
  const int kth = (lane & 48) | (k - 1);  // the lane of this DPP row that holds slot k - 1
  for (int j0 = 0; j0 < C; j0 += TB) {
    const float* pb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) pb[p] = lab + (long)min(j0 + p * 16 + srow, C - 1) * E + sj * 4;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    raw_t va[4];
    float4 vb[4];
    loada(va, pa, 0);
    loadb(vb, pb, 0);
    for (int k0 = 0; k0 < E; k0 += TK) {
      __syncthreads();
      {
        float4 wa[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) wa[p] = gal_widen<GT>(va[p]);
        put(stage[0], wa);
      }
      put(stage[1], vb);
      __syncthreads();
      if (k0 + TK < E) {
        loada(va, pa, k0 + TK);
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
    // C[row = 4 * qd + e][label = j0 + 16 t + r]: labels past C are out of the selection and of the softmax
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = j0 + t * 16 + r;
      uint64_t ckey[4];
      float cs[4];
      unsigned pend = 0;  // bit e: this lane's candidate of row e passes
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cs[e] = fmaf(acc[t][e], scale, bias);
        ckey[e] = col < C ? topk_key(__float_as_uint(cs[e]), (uint32_t)col) : 0;
        if constexpr (SOFTMAX)
          if (col < C) ms_add(m[e], s[e], cs[e]);
        pend |= (ckey[e] > cut[e] ? 1u : 0u) << e;
      }
      if (__ballot(pend != 0) == 0) continue;  // wave-uniform
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bool mine = (pend >> e) & 1u;
        uint64_t bal = __ballot(mine);
        if (bal == 0) continue;
        do {  // wave-uniform: one candidate per DPP row and turn
          const unsigned grp = (unsigned)(bal >> (lane & 48)) & 0xffffu;  // this row's lanes with a candidate
          const int src = (lane & 48) | (grp ? __builtin_ctz(grp) : 0);
          const uint64_t ck = __shfl((unsigned long long)ckey[e], src, 64);
          const float cf = __shfl(cs[e], src, 64);
          list_insert(lkey[e], lscore[e], grp ? ck : 0, cf);
          if (lane == src) mine = false;
          bal = __ballot(mine);
        } while (bal != 0);
        cut[e] = __shfl((unsigned long long)lkey[e], kth, 64);
      }
    }
  }
  // lane r writes slot r of its four rows
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float2 ms = make_float2(kNegInf, 0.f);
    if constexpr (SOFTMAX) {
      ms = ms_group16(m[e], s[e]);
      if (ms.x == INFINITY) ms.y = NAN;  // exp(inf - inf), as the search's merge
    }
    const int in = rowbase + 4 * qd + e;  // the row inside the tile
    const unsigned row = i0 + in;
    if (row >= (unsigned)N) continue;
    const bool allowed = (((in < 32 ? mw.x : mw.y) >> (in & 31)) & 1u) != 0;
    const bool empty = !allowed || lkey[e] == 0;
    if (r < k) {
      const long at = (long)row * k + r;
      const float l = lscore[e];
      label[at] = empty ? -1 : (int32_t)~(uint32_t)lkey[e];
      score[at] = empty ? kNegInf : l;
      if constexpr (SOFTMAX)
        prob[at] = empty ? 0.f : expf(l - ms.x) / ms.y;
      else
        prob[at] = empty ? 0.f : 1.0f / (1.0f + expf(-l));
    }
    if (SOFTMAX && norm && r == 0) {
      norm[2 * (long)row] = allowed ? ms.x : kNegInf;
      norm[2 * (long)row + 1] = allowed ? ms.y : 0.f;
    }
  }
}

template <typename GT, bool MASKED, bool SOFTMAX>
void launch_classify_of(const ClassifyArgs& a) {
  hipLaunchKernelGGL((classify_kernel<GT, MASKED, SOFTMAX>), dim3((a.N + TB - 1) / TB), dim3(256), 0, a.stream,
                     (const GT*)a.g, a.labels, a.N, a.C, a.E, a.k, a.scale, a.bias, (const uint2*)a.mask, a.label,
                     a.score, a.prob, a.norm);
}

// Every instantiation: [gallery type][MASKED][softmax].
typedef void (*ClassifyLaunch)(const ClassifyArgs&);
#define CLASSIFY_M(GT, M) { launch_classify_of<GT, M, false>, launch_classify_of<GT, M, true> }
#define CLASSIFY_GT(GT) { CLASSIFY_M(GT, false), CLASSIFY_M(GT, true) }
constexpr ClassifyLaunch kClassify[3][2][2] = {CLASSIFY_GT(float), CLASSIFY_GT(_Float16), CLASSIFY_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kClassify");

}  // namespace

hipError_t launch_classify(const ClassifyArgs& a) {
  if (a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.C < 1 || a.C > kClusterMaxCentroids) return hipErrorInvalidValue;
  if (a.k < 1 || a.k > kClassifyMaxK || (a.probs != TOPK_PROBS_SOFTMAX && a.probs != TOPK_PROBS_SIGMOID))
    return hipErrorInvalidValue;
  if (!a.g || !a.labels || !a.label || !a.score || !a.prob) return hipErrorInvalidValue;
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  if (((uintptr_t)a.labels & 15) || (a.mask && ((uintptr_t)a.mask & 7))) return hipErrorInvalidValue;
  kClassify[a.dtype][a.mask != nullptr][a.probs == TOPK_PROBS_SOFTMAX](a);
  return hipGetLastError();
}

}  // namespace clipgpu
