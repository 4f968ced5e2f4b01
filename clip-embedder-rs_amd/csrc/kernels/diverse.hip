// Diversified search of the embedding index (clipgpu_index_search_diverse): maximal marginal relevance over the
// pool of a search's P best rows, on the device.  The pool (ids c[t], logits l[t], t < P <= 128) is launch_topk's
// result; this unit re-ranks it:
//
//   G[t][u] = fmaf(dot(row c[t], row c[u]), scale, bias)           similarity's bits, rows as stored
//   step 0 takes candidate 0; after taking s, m[t] = G[s][t] where that is greater (a NaN never is);
//   step j takes the open candidate with the best v[t] = a l[t] - lam m[t], a = 1 - lam, every operation rounded
//   once, in the order of topk_key.hpp on v (descending, NaN last), equal v by the lower t.
//   out[j] = (c[s_j], l[s_j]); (-1, -inf) once the real candidates are used up.
//
// Gram kernel (diverse_gram_kernel).  Grid (tile pair, query); block: ONE wave, one 16 x 16 tile of G, rows from
// the 16-candidate panel ta, columns from panel tb >= ta.  The lanes gather the two panels' rows through the
// pool's ids straight from the gallery in its storage type (lane -> rows lane / 16 + 4 p, p < 4; k quad lane % 16:
// a 64-wide k slab is one 16-byte load per row, 8 bytes for a 16-bit gallery, widened in registers), stage them in
// the [row][k slot][k step] layout of topk_stage.hpp and run the v_mfma_f32_16x16x4_f32 chain over them with k
// ascending, MFMA i on k = 4 i .. 4 i + 3: similarity's chain, so G has its bits.  The next slab's loads are
// issued before the chain of the slab in hand.  E % 16 == 0; a last slab shorter than 64 runs only its E % 64 / 4
// steps (its other staged columns hold clamped loads that no MFMA reads), so no zero is ever added to a sum.
// A diagonal pair stages one panel and reads it as both operands.  The epilogue is one fmaf and two stores, the
// second mirrored: G is bit-symmetric (the products commute, the k order is the same), so only pairs on or above
// the diagonal run -- T (T + 1) / 2 blocks per query, 36 at P = 128, which spreads ONE query over 36 CUs where a
// block per query would run ~2,000 dependent MFMAs on one.  A candidate that is padding (id -1) or past P is not
// gathered, and a pair with a panel of only such candidates leaves; their entries of G are never read.
//   LDS 11,264 bytes (2 panels x 16 rows x 88 floats); no block barrier (one wave).
//
// Greedy kernel (diverse_greedy_kernel).  One wave per query, four per block, no block barrier and no LDS.  Lane x
// owns candidates x and x + 64: id, l, m and the open flag live in registers.  A step: each lane's better key, two
// wave-wide u32 max reductions (DPP row rotations, then lane ^ 16 and lane ^ 32) -- the largest w = topk_mono(v) + 1
// (0: not open), then the largest ~t among the lanes that hold it --, lane 0 writes the output, and one coalesced
// read of row s of G (P floats, 512 bytes at most) updates m.  k steps, each one dependent L2 round trip.
//
// Built with packed-f32 instruction selection off (Makefile): the bits of v decide the result.
#include <cstdint>

#include "common.hpp"
#include "gallery.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

template <typename GT>
__global__ __launch_bounds__(64) void diverse_gram_kernel(const GT* __restrict__ gal, int N, int E, int P, int T,
                                                          float scale, float bias,
                                                          const int64_t* __restrict__ pool_idx,
                                                          float* __restrict__ gram) {
  typedef typename GalRaw<GT>::type raw_t;
  __shared__ __attribute__((aligned(16))) float stage[2][NB * LDT];  // panel ta | panel tb: [row][k slot qd][k step]
  const int lane = threadIdx.x, q = blockIdx.y;
  int ta = 0, tb = blockIdx.x;  // pair -> (ta, tb), ta <= tb < T: row ta of the upper triangle holds T - ta pairs
  while (tb >= T - ta) {
    tb -= T - ta;
    ++ta;
  }
  tb += ta;
  const bool diag = ta == tb;
  const int64_t* ids = pool_idx + (long)q * P;
  const int srow = lane >> 4, sj = lane & 15;
  const GT* pa[4];
  const GT* pb[4];
  bool oka[4], okb[4], any_a = false, any_b = false;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int t = ta * NB + p * 4 + srow, u = tb * NB + p * 4 + srow;
    const int64_t ia = t < P ? ids[t] : -1, ib = u < P ? ids[u] : -1;
    oka[p] = ia >= 0 && ia < N;
    okb[p] = !diag && ib >= 0 && ib < N;
    pa[p] = gal + (oka[p] ? ia : 0) * (long)E;
    pb[p] = gal + (okb[p] ? ib : 0) * (long)E;
    any_a |= oka[p];
    any_b |= diag ? oka[p] : okb[p];
  }
  if (__ballot(any_a) == 0 || __ballot(any_b) == 0) return;  // wave-uniform: a panel of padding only
  raw_t va[4] = {}, vb[4] = {};
  auto request = [&](int ck) {  // the slab at k = ck: this lane's quad, clamped into the row
    const int ko = min(ck + sj * 4, E - 4);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (oka[p]) va[p] = gal_raw(pa[p] + ko);
      if (okb[p]) vb[p] = gal_raw(pb[p] + ko);
    }
  };
  auto put = [&](float* dst, int p, float4 v) {
    float* d = dst + (p * 4 + srow) * LDT + sj;
    d[0] = v.x; d[KQ] = v.y; d[2 * KQ] = v.z; d[3 * KQ] = v.w;
  };
  const int r = lane & 15, qd = lane >> 4;
  // 16x16x4: lane (r, qd) supplies A[r][qd] and B[qd][r]; k = ck + 4 * (4 jq + st) + qd, ascending
  const float* fa = &stage[0][r * LDT + qd * KQ];
  const float* fb = &stage[diag ? 0 : 1][r * LDT + qd * KQ];
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  request(0);
  for (int ck = 0; ck < E; ck += TK) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      put(stage[0], p, gal_widen<GT>(va[p]));
      if (!diag) put(stage[1], p, gal_widen<GT>(vb[p]));
    }
    wave_lds_order();
    if (ck + TK < E) request(ck + TK);  // in flight during the chain below
    const int quads = min(TK, E - ck) / 16;  // E % 16 == 0: 1 .. 4 groups of four MFMA steps
    for (int jq = 0; jq < quads; ++jq) {
      const f32x4 a = *(const f32x4*)(fa + jq * 4);
      const f32x4 b = *(const f32x4*)(fb + jq * 4);
#pragma unroll
      for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st], b[st], acc, 0, 0, 0);
    }
    wave_lds_order();  // the fragment reads come before the next slab's stores
  }
  // C[row = 4 * qd + e][col = r]
  float* G = gram + (long)q * P * P;
  const int u = tb * NB + r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int t = ta * NB + 4 * qd + e;
    if (t < P && u < P) {
      const float g = fmaf(acc[e], scale, bias);
      G[t * P + u] = g;
      if (!diag) G[u * P + t] = g;
    }
  }
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = max(v, dpp_u32<0x128>(v));  // row_ror:8, 4, 2, 1: the 16 lanes of a row
  v = max(v, dpp_u32<0x124>(v));
  v = max(v, dpp_u32<0x122>(v));
  v = max(v, dpp_u32<0x121>(v));
  v = max(v, (uint32_t)__shfl_xor((int)v, 16));
  v = max(v, (uint32_t)__shfl_xor((int)v, 32));
  return v;
}

// v = a l - lam m: two products and a difference, each rounded once.  The toolchain contracts a * b - c * d into an
// fma by default (and __fmul_rn / __fsub_rn are plain operators to it), so contraction is switched off here.
__device__ __forceinline__ float mmr_value(float a, float l, float lam, float m) {
#pragma clang fp contract(off)
  const float rel = a * l, red = lam * m;
  return rel - red;
}

__global__ __launch_bounds__(256) void diverse_greedy_kernel(int nq, int N, int P, int k, float lam,
                                                             const int64_t* __restrict__ pool_idx,
                                                             const float* __restrict__ pool_score,
                                                             const float* __restrict__ gram,
                                                             int64_t* __restrict__ out_idx,
                                                             float* __restrict__ out_score) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;  // whole waves leave; the kernel has no block barrier
  const float a = 1.0f - lam;
  int id[2];  // a pool id is a gallery row, below 2^31; -1 = not a candidate
  float l[2], m[2];
  bool open[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int t = lane + 64 * h;
    const int64_t c = t < P ? pool_idx[(long)q * P + t] : -1;
    id[h] = c >= 0 && c < N ? (int)c : -1;
    l[h] = t < P ? pool_score[(long)q * P + t] : -INFINITY;
    m[h] = -INFINITY;
    open[h] = id[h] >= 0;
  }
  const float* G = gram + (long)q * P * P;
  int64_t* oi = out_idx + (long)q * k;
  float* os = out_score + (long)q * k;
  int s = 0;  // step 0 takes candidate 0
  bool any = __shfl(id[0], 0) >= 0;
  for (int j = 0; j < k; ++j) {
    if (j > 0) {
      uint32_t w = 0, nt = 0;  // this lane's better candidate: w = topk_mono(v) + 1 (at most 0xff800001), nt = ~t
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float v = mmr_value(a, l[h], lam, m[h]);
        const uint32_t wh = open[h] ? topk_mono(__float_as_uint(v)) + 1u : 0u;
        if (wh > w) {  // equal w: the lower t, slot 0, stays
          w = wh;
          nt = ~(uint32_t)(lane + 64 * h);
        }
      }
      const uint32_t best = wave_max_u32(w);
      any = best != 0;
      s = (int)~wave_max_u32(w == best ? nt : 0u);  // the lowest t among the lanes that hold the best v
    }
    if (!any) {  // the real candidates are used up
      for (int t = j + lane; t < k; t += 64) {
        oi[t] = -1;
        os[t] = -INFINITY;
      }
      break;
    }
    const int h = s >> 6, src = s & 63;  // wave-uniform
    const int sid = __shfl(h ? id[1] : id[0], src);
    const float sl = __shfl(h ? l[1] : l[0], src);
    if (lane == 0) {
      oi[j] = sid;
      os[j] = sl;
    }
    if (lane == src) open[h] = false;
    if (j + 1 < k) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        if (open[hh]) {  // open: a real candidate below P, whose entry the Gram kernel wrote
          const float g = G[s * P + lane + 64 * hh];
          if (g > m[hh]) m[hh] = g;
        }
    }
  }
}

template <typename GT>
void launch_gram(const DiverseArgs& a, int T) {
  hipLaunchKernelGGL((diverse_gram_kernel<GT>), dim3(T * (T + 1) / 2, a.nq), dim3(64), 0, a.stream, (const GT*)a.g, a.N,
                     a.E, a.P, T, a.scale, a.bias, a.pool_idx, a.gram);
}

}  // namespace

hipError_t launch_diverse(const DiverseArgs& a) {
  if (!a.g || !a.pool_idx || !a.pool_score || !a.gram || !a.out_idx || !a.out_score) return hipErrorInvalidValue;
  if (a.nq <= 0 || a.nq > 65535 || a.N <= 0 || a.E <= 0 || a.E % 16 != 0) return hipErrorInvalidValue;
  if (a.P < 1 || a.P > kTopkMax || a.k < 1 || a.k > a.P) return hipErrorInvalidValue;
  if (!(a.lam >= 0.0f && a.lam <= 1.0f)) return hipErrorInvalidValue;
  if (((uintptr_t)a.g & 15) || ((uintptr_t)a.gram & 3)) return hipErrorInvalidValue;
  const int T = (a.P + NB - 1) / NB;
  if (a.dtype == TOPK_GAL_F32) launch_gram<float>(a, T);
  else if (a.dtype == TOPK_GAL_F16) launch_gram<_Float16>(a, T);
  else if (a.dtype == TOPK_GAL_BF16) launch_gram<__bf16>(a, T);
  else return hipErrorInvalidValue;
  hipLaunchKernelGGL(diverse_greedy_kernel, dim3((a.nq + 3) / 4), dim3(256), 0, a.stream, a.nq, a.N, a.P, a.k, a.lam,
                     a.pool_idx, a.pool_score, a.gram, a.out_idx, a.out_score);
  return hipGetLastError();
}

}  // namespace clipgpu
