// Assignment and k-means over a device-resident gallery (clipgpu_index_assign[_device], clipgpu_index_kmeans).
//
//   assign_kernel         label[j] = the centroid with the largest topk_key(score, centroid index) for gallery
//                         row j, score = fmaf(dot(c, g[j]), scale, bias): the range search's 64 x 64 tile loop
//                         (range_wide_kernel: the same v_mfma_f32_16x16x4_f32 chain in the same k order through
//                         the same [k slot][k step] staging, so a score carries the search's bits) with the
//                         gallery rows on the A side and another selection.  A block owns 64 gallery rows and
//                         walks every 64-centroid tile; each row's running best (key, score) stays in registers
//                         -- in-lane over the tile's four columns, then across the 16 lanes that share the row
//                         -- so there is no LDS list, no candidate buffer and no merge.
//   cluster_stats_kernel  max |x| (as a max over f32 bit patterns), the first row with a non-finite element and
//                         the number of live allowed rows: what the update's shift is made of.
//   cluster_moved_kernel  how many rows changed their label between two generations.
//   cluster_sums_kernel   S[c][i] += llrint(ldexp((double)g[j][i], shift)) over the rows labelled c: 64-bit
//                         integer vector atomics, one wave instruction = 64 consecutive columns of one row of
//                         S (512 contiguous bytes).  Integer adds commute exactly: the sums do not depend on
//                         the order rows are met in.
//   cluster_finalise_kernel  centroid[c] = S[c] / ||S[c]|| in f64 with the sum of squares taken sequentially,
//                         i ascending, multiply and add kept apart; a cluster whose sums are all zero (no
//                         member, or members that cancel) keeps its centroid.
//   gal_gather_kernel     rows at given ids, widened to f32 (clipgpu_index_get_rows_at).
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

constexpr float kNegInf = -__builtin_huge_valf();

// Block: 64 gallery rows (A) x every centroid (B) in tiles of 64, as range_wide_kernel.  44 KiB of LDS.
template <typename GT, bool MASKED>
__global__ __launch_bounds__(256, 3) void assign_kernel(const GT* __restrict__ gal, const float* __restrict__ cen, int N,
                                                        int C, int E, float scale, float bias,
                                                        const uint2* __restrict__ mask, int32_t* __restrict__ label,
                                                        float* __restrict__ score) {
  __shared__ __attribute__((aligned(16))) float stage[2][TB * LDT];  // A | B: [row][k slot qd][k step]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // rows as unsigned: N < 2^31, but the last tile's padding rows may reach 2^31
  const unsigned i0 = blockIdx.x * (unsigned)TB;
  uint2 mw = make_uint2(~0u, ~0u);  // the tile's allowed bits: rows i0 .. i0 + 31 | i0 + 32 .. i0 + 63
  if constexpr (MASKED) {
    mw = mask[blockIdx.x];
    if ((mw.x | mw.y) == 0) {  // block-uniform: no allowed row, the empty entry for every row in range
      if (tid < TB && i0 + tid < (unsigned)N) {
        label[i0 + tid] = -1;
        score[i0 + tid] = kNegInf;
      }
      return;
    }
  }
  const int rowbase = wave * 16;
  const int r = lane & 15, qd = lane >> 4;
  // Staging: as range_wide_kernel (thread -> rows tid / 16 + 16 p, k step tid % 16; the next slab's loads are
  // issued before this slab's MFMAs), with the gallery on the A side.
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
  // rows rowbase + 4 * qd + e: the running best of each, key 0 = nothing yet (topk_key.hpp's empty slot)
  uint64_t best[4] = {0, 0, 0, 0};
  float bscore[4] = {kNegInf, kNegInf, kNegInf, kNegInf};
  for (int j0 = 0; j0 < C; j0 += TB) {
    const float* pb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) pb[p] = cen + (long)min(j0 + p * 16 + srow, C - 1) * E + sj * 4;
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
    // C[row = 4 * qd + e][centroid = j0 + 16 t + r]: centroids past C are out of the selection
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = j0 + t * 16 + r;
      if (col < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s = fmaf(acc[t][e], scale, bias);
          const uint64_t key = topk_key(__float_as_uint(s), (uint32_t)col);
          if (key > best[e]) {
            best[e] = key;
            bscore[e] = s;
          }
        }
      }
    }
  }
  // across the 16 lanes (r) that hold a row: keys are unique per centroid, so the largest has one score
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const uint64_t ok = __shfl_xor((unsigned long long)best[e], m, 64);
      const float os = __shfl_xor(bscore[e], m, 64);
      if (ok > best[e]) {
        best[e] = ok;
        bscore[e] = os;
      }
    }
  }
  if (r == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int in = rowbase + 4 * qd + e;  // the row inside the tile
      const unsigned row = i0 + in;
      if (row >= (unsigned)N) continue;
      const bool allowed = (((in < 32 ? mw.x : mw.y) >> (in & 31)) & 1u) != 0;
      label[row] = allowed ? (int32_t)~(uint32_t)best[e] : -1;  // key 0: ~0 = -1 too
      score[row] = allowed ? bscore[e] : kNegInf;
    }
  }
}

template <typename GT, bool MASKED>
void launch_assign_of(const AssignArgs& a) {
  hipLaunchKernelGGL((assign_kernel<GT, MASKED>), dim3((a.N + TB - 1) / TB), dim3(256), 0, a.stream, (const GT*)a.g, a.c,
                     a.N, a.C, a.E, a.scale, a.bias, (const uint2*)a.mask, a.label, a.score);
}

// Every instantiation: [gallery type][MASKED].
typedef void (*AssignLaunch)(const AssignArgs&);
#define ASSIGN_GT(GT) { launch_assign_of<GT, false>, launch_assign_of<GT, true> }
constexpr AssignLaunch kAssign[3][2] = {ASSIGN_GT(float), ASSIGN_GT(_Float16), ASSIGN_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kAssign");

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = max(v, (unsigned)__shfl_xor((int)v, m, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
  return v;
}

__device__ __forceinline__ bool row_allowed(const uint32_t* mask, int row) {
  return !mask || ((mask[row >> 5] >> (row & 31)) & 1u) != 0;
}

// A block takes rows blockIdx.x, + gridDim.x, ...; a thread four elements of a row per step.
template <typename GT>
__global__ __launch_bounds__(256) void cluster_stats_kernel(const GT* __restrict__ gal, int N, int E4,
                                                            const uint32_t* __restrict__ mask, ClusterStat* stat) {
  unsigned mx = 0, bad = 0, n = 0;  // bad: ~row of the first row with a non-finite element, 0 = none
  for (int row = blockIdx.x; row < N; row += gridDim.x) {
    if (!row_allowed(mask, row)) continue;  // block-uniform
    if (threadIdx.x == 0) ++n;
    unsigned m = 0;
    for (int c = threadIdx.x; c < E4; c += 256) {
      const float4 v = gal_widen<GT>(gal_raw(gal + ((long)row * E4 + c) * 4));
      m = max(max(m, __float_as_uint(v.x) & 0x7fffffffu), __float_as_uint(v.y) & 0x7fffffffu);
      m = max(max(m, __float_as_uint(v.z) & 0x7fffffffu), __float_as_uint(v.w) & 0x7fffffffu);
    }
    if (m >= 0x7f800000u) bad = max(bad, ~(unsigned)row);
    mx = max(mx, m);
  }
  mx = wave_max_u32(mx);
  bad = wave_max_u32(bad);
  n = wave_sum_u32(n);
  if ((threadIdx.x & 63) == 0) {
    if (mx) atomicMax(&stat->max_bits, mx);
    if (bad) atomicMax(&stat->bad_row, bad);
    if (n) atomicAdd(&stat->n, n);
  }
}

// A live allowed row has a label >= 0 (C >= 1: some key is above the empty one), every other row -1.
__global__ __launch_bounds__(256) void cluster_moved_kernel(const int32_t* __restrict__ cur,
                                                            const int32_t* __restrict__ prev, int N,
                                                            unsigned long long* moved) {
  unsigned n = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const int32_t c = cur[i];
    n += c >= 0 && c != prev[i];
  }
  n = wave_sum_u32(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(moved, (unsigned long long)n);
}

// A block takes a run of rows; thread t the columns t, t + 256, ...: a wave's 64 adds of one step are 512
// contiguous bytes of one row of S.  Four rows are in flight per step (their loads go out together).
template <typename GT>
__global__ __launch_bounds__(256) void cluster_sums_kernel(const GT* __restrict__ gal, const int32_t* __restrict__ label,
                                                           int N, int E, int shift, int rows_per_block,
                                                           unsigned long long* __restrict__ S) {
  const long first = (long)blockIdx.x * rows_per_block;
  const long last = min((long)N, first + rows_per_block);
  for (long row = first; row < last; row += 4) {
    int c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) c[u] = row + u < last ? label[row + u] : -1;  // block-uniform
    for (int col = threadIdx.x; col < E; col += 256) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = c[u] >= 0 ? (float)gal[(row + u) * E + col] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c[u] >= 0) {
          // exact scaling in f64, then round to nearest even; |value| < 2^62 by the choice of the shift
          const long long q = __double2ll_rn(ldexp((double)v[u], shift));
          atomicAdd(&S[(long)c[u] * E + col], (unsigned long long)q);
        }
    }
  }
}

// One wave per centroid.  Every lane takes the same sequential sum of squares (the loads are broadcasts), then
// the lanes share the columns.
__global__ __launch_bounds__(64) void cluster_finalise_kernel(const long long* __restrict__ S, int E,
                                                              float* __restrict__ cen) {
#pragma clang fp contract(off)
  const long long* s = S + (long)blockIdx.x * E;
  double n2 = 0.0;
  for (int i = 0; i < E; ++i) {
    const double v = (double)s[i];
    n2 = __dadd_rn(n2, __dmul_rn(v, v));
  }
  if (!(n2 > 0.0)) return;  // no member, or members that cancel: the centroid stays
  const double norm = __dsqrt_rn(n2);
  for (int i = threadIdx.x; i < E; i += 64) cen[(long)blockIdx.x * E + i] = (float)__ddiv_rn((double)s[i], norm);
}

template <typename GT>
__global__ __launch_bounds__(256) void gal_gather_kernel(const GT* __restrict__ gal, const int64_t* __restrict__ ids,
                                                         float* __restrict__ out, long n, int E4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n * E4; i += (long)gridDim.x * 256) {
    const long row = i / E4, c = i - row * E4;
    ((float4*)out)[i] = gal_widen<GT>(gal_raw(gal + (ids[row] * E4 + c) * 4));
  }
}

bool gal_type(int dtype) { return dtype == TOPK_GAL_F32 || dtype == TOPK_GAL_F16 || dtype == TOPK_GAL_BF16; }

}  // namespace

hipError_t launch_assign(const AssignArgs& a) {
  if (a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.C < 1 || a.C > kClusterMaxCentroids) return hipErrorInvalidValue;
  if (!a.g || !a.c || !a.label || !a.score || !gal_type(a.dtype)) return hipErrorInvalidValue;
  if (((uintptr_t)a.c & 15) || (a.mask && ((uintptr_t)a.mask & 7))) return hipErrorInvalidValue;
  kAssign[a.dtype][a.mask != nullptr](a);
  return hipGetLastError();
}

hipError_t launch_cluster_stats(const void* g, int dtype, int N, int E, const uint32_t* mask, ClusterStat* stat,
                                hipStream_t s) {
  if (N <= 0 || E <= 0 || E % 4 || !g || !stat || !gal_type(dtype)) return hipErrorInvalidValue;
  const dim3 grid(std::min(N, 2048));
  if (dtype == TOPK_GAL_F32)
    hipLaunchKernelGGL(cluster_stats_kernel<float>, grid, dim3(256), 0, s, (const float*)g, N, E / 4, mask, stat);
  else if (dtype == TOPK_GAL_F16)
    hipLaunchKernelGGL(cluster_stats_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)g, N, E / 4, mask, stat);
  else
    hipLaunchKernelGGL(cluster_stats_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)g, N, E / 4, mask, stat);
  return hipGetLastError();
}

hipError_t launch_cluster_moved(const int32_t* cur, const int32_t* prev, int N, unsigned long long* moved,
                                hipStream_t s) {
  if (N <= 0 || !cur || !prev || !moved || ((uintptr_t)moved & 7)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cluster_moved_kernel, dim3(std::min((N + 255) / 256, 1024)), dim3(256), 0, s, cur, prev, N, moved);
  return hipGetLastError();
}

hipError_t launch_cluster_sums(const void* g, int dtype, const int32_t* label, int N, int E, int shift, int64_t* S,
                               hipStream_t s) {
  if (N <= 0 || E <= 0 || !g || !label || !S || ((uintptr_t)S & 7) || !gal_type(dtype)) return hipErrorInvalidValue;
  const int rows_per_block = std::max(16, (N + 8191) / 8192);
  const dim3 grid((N + rows_per_block - 1) / rows_per_block);
  unsigned long long* u = (unsigned long long*)S;
  if (dtype == TOPK_GAL_F32)
    hipLaunchKernelGGL(cluster_sums_kernel<float>, grid, dim3(256), 0, s, (const float*)g, label, N, E, shift,
                       rows_per_block, u);
  else if (dtype == TOPK_GAL_F16)
    hipLaunchKernelGGL(cluster_sums_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)g, label, N, E, shift,
                       rows_per_block, u);
  else
    hipLaunchKernelGGL(cluster_sums_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)g, label, N, E, shift,
                       rows_per_block, u);
  return hipGetLastError();
}

hipError_t launch_cluster_finalise(const int64_t* S, int C, int E, float* cen, hipStream_t s) {
  if (C < 1 || C > kClusterMaxCentroids || E <= 0 || !S || !cen) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cluster_finalise_kernel, dim3(C), dim3(64), 0, s, (const long long*)S, E, cen);
  return hipGetLastError();
}

hipError_t launch_gal_gather(int dtype, const void* gal, const int64_t* ids, float* out, long n, int E, hipStream_t s) {
  if (n <= 0 || E <= 0 || E % 4 || !gal || !ids || !out || !gal_type(dtype)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)std::min<long>((n * (E / 4) + 255) / 256, 8192));
  if (dtype == TOPK_GAL_F32)
    hipLaunchKernelGGL(gal_gather_kernel<float>, grid, dim3(256), 0, s, (const float*)gal, ids, out, n, E / 4);
  else if (dtype == TOPK_GAL_F16)
    hipLaunchKernelGGL(gal_gather_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)gal, ids, out, n, E / 4);
  else
    hipLaunchKernelGGL(gal_gather_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)gal, ids, out, n, E / 4);
  return hipGetLastError();
}

}  // namespace clipgpu
