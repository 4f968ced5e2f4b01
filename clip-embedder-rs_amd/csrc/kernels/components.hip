// Duplicate groups of the embedding index (clipgpu_index_components): the connected components of the threshold
// graph, one label per row, with no pair list.
//
//   vertices = the live allowed rows
//   edge i-j = fmaf(dot(g[i], g[j]), scale, bias) >= threshold as f32   the score bits and the comparison of the
//                                                                        self-join (kernels/range.hip); no NaN passes
//   label[i] = the smallest row id of i's component, -1 for a row that is dead or not allowed
//
// Three launches on one stream, nothing read back between them.
//
// 1. cc_init_kernel: parent[i] = i for every slot below N, and the component counter to zero.
//
// 2. cc_join_kernel, the tile work of the self-join with another operand path and another epilogue.  A block is one
//    panel of 64 rows (4 waves x 16 rows) against one span of 64-column tiles.  BOTH operands are loaded from the
//    gallery in its own element type (gal_raw), kept as loaded while the loads are in flight and widened when they
//    are staged (gal_widen), as kernels/knn.hip loads its A operand: no f32 copy of the rows, no widening pass, no
//    host loop over chunks.  The v_mfma_f32_16x16x4_f32 chain starts from zero and runs k ascending through the
//    [k slot][k step] staging of topk_stage.hpp, so a score carries the self-join's bits.
//
//    Grid.  Panel p (rows 64 p ..) needs the column tiles p .. n_tiles - 1: w = n_tiles - p of them, so the upper
//    triangle is n_tiles (n_tiles + 1) / 2 tiles.  A panel whose only tile holds no column above its first row (the
//    last one, when N = 64 p + 1) is not enumerated.  With a span length of T tiles a panel is cut into
//    ceil(w / T) spans of ceil(w / spans) tiles each, and panels of equal span count form a group of T panels.  A
//    block of a panel with two or more spans does between T / 2 and T tiles; the last T panels (the first group,
//    one span each) are the tail, blocks of 1 .. T tiles.  The grid is one-dimensional; a block finds its group from its
//    index in closed form (a square root and two corrections, scalar work), so there is no table to upload.
//    Within a group the panel runs fastest: the blocks dispatched together are neighbouring panels at the same
//    span index, whose column ranges overlap but for one tile per panel, so they read the same gallery tiles.
//    How T was chosen: T = ceil(triangle / 4096), at most 32.  A tile at E = 512 is eight slabs of 16 MFMA steps
//    per wave; 32 of them keep a block busy long enough that the launch of its successor costs nothing, while 4096
//    blocks and more are five rounds of the 768 blocks the chip holds (256 CUs x 3 blocks at 44 KiB of LDS), so
//    the half-length blocks at the ends of the groups and the short blocks of the tail even out.  Below 4096 x 32 tiles (N below ~33 000) T shrinks
//    so that the grid still has ~4096 blocks, down to one tile per block.  The g_topk_span_cols hook, when set,
//    is T in columns.  Nothing in the result depends on T.
//
//    Epilogue.  A column j passes for row i only if j > i, j < N and both are live and allowed (the effective mask
//    words of the search; MASKED is a template parameter).  A wave ballot of "any hit" is zero for nearly every
//    tile, and then nothing happens.  Otherwise a lane loads parent[] once for each of its rows and columns that
//    has a hit, and every hit whose two entries differ goes through uf_unite.  In a large cluster nearly every hit
//    leaves at that comparison.  No records, no counter.
//
//    Union-find, lock-free, THE SMALLER ID ALWAYS THE ROOT.  Every write to parent[] is either
//    atomicCAS(&parent[big], big, small) with small < big both roots of components an edge joins, or an atomicMin
//    with an ancestor.  So parent[x] only ever decreases, parent[x] <= x, and parent[x] always names a row of x's
//    component: the structure is a forest at every instant and uf_find terminates.  A CAS fails only because
//    another hook of the same root succeeded, and there are fewer than N hooks in all, so uf_unite terminates.
//    When the kernel has finished, every edge's end points share a root, and a root is the smallest id of its
//    tree, hence of its component: the labels are a function of the inputs alone, whatever order the blocks ran in.
//
// 3. cc_flatten_kernel: label[i] = uf_find(i) for a live allowed row, else -1; the counter counts label[i] == i
//    (one atomic per wave).  When asked it also writes the group labels kernels/grouped.hip reads: the component's
//    label for a live allowed row, "ungrouped" (0x80000000 | slot) for every other slot below N.
//
// LDS: the staging alone, 44 KiB, three blocks per CU as the self-join's wide kernel.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "gallery.hpp"
#include "kernels.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

constexpr int kCcBlocks = 4096;               // the blocks a call is cut into, where the triangle has the tiles
constexpr int kCcSpanTiles = 32;              // the longest span, in tiles
constexpr uint32_t kUngrouped = 0x80000000u;  // | slot: the group label of a row without one (kernels/grouped.hip)

__device__ __forceinline__ int uf_load(const int* parent, unsigned x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree.  A node whose parent is not a root is moved under its grandparent on the way.
__device__ __forceinline__ int uf_find(int* parent, int x) {
  int p = uf_load(parent, x);
  while (p != x) {
    const int gp = uf_load(parent, p);
    if (gp != p) atomicMin(parent + x, gp);
    x = p;
    p = gp;
  }
  return x;
}

// Joins the trees of a and b: the larger root is hooked under the smaller.
__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int small = min(a, b), big = max(a, b);
    if (atomicCAS(parent + big, big, small) == big) return;
    a = small;  // big was hooked elsewhere meanwhile: again, from the two roots
    b = big;
  }
}

__global__ __launch_bounds__(256) void cc_init_kernel(int* __restrict__ parent, int N, unsigned* __restrict__ count) {
  if (count && blockIdx.x == 0 && threadIdx.x == 0) *count = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) parent[i] = (int)i;
}

// The cut of the triangle: T tiles per span at most; blocks [0, T m (m + 1) / 2 + ...) in groups m = 0, 1, ... of
// T panels with m + 1 spans each, counted from the LAST panel (q = n_tiles - 1 - p, w = q + 1 tiles).
struct CcCut { int n_tiles, T; long first, blocks; };  // first: the blocks left out in front (0 or 1)

template <typename GT, bool MASKED>
__global__ __launch_bounds__(256, 3) void cc_join_kernel(const GT* __restrict__ gal, int N, int E, float scale, float bias,
                                                         float thr, CcCut cut, const uint2* __restrict__ mask,
                                                         int* __restrict__ parent) {
  typedef typename GalRaw<GT>::type raw_t;
  __shared__ __attribute__((aligned(16))) float stage[2][TB * LDT];  // A | B: [row][k slot qd][k step]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // block -> (group m, panel q of the group, span): all block-uniform
  const long T = cut.T, b = (long)blockIdx.x + cut.first;
  long m = (long)((sqrt(1.0 + 8.0 * (double)b / (double)T) - 1.0) * 0.5);
  while (m > 0 && T * m * (m + 1) / 2 > b) --m;
  while (T * (m + 1) * (m + 2) / 2 <= b) ++m;
  const long rest = b - T * m * (m + 1) / 2;
  const long in_group = min(T, (long)cut.n_tiles - m * T);  // the last group may be short
  const int q = (int)(m * T + rest % in_group), span = (int)(rest / in_group);
  const int panel = cut.n_tiles - 1 - q, w = q + 1, spans = (int)m + 1;
  const int len = (w + spans - 1) / spans;
  const int i0 = panel * TB;
  // columns as unsigned: N < 2^31, but the last tile's padding columns may reach 2^31
  const unsigned c_begin = (unsigned)(panel + span * len) * TB;
  const unsigned c_end = min((unsigned)N, (unsigned)(panel + min((span + 1) * len, w)) * TB);
  if (c_begin >= c_end) return;
  if constexpr (MASKED) {  // a panel with no allowed row or a span with no allowed column (block-uniform)
    const uint2 pm = mask[panel];
    unsigned any = 0;
    for (unsigned t = (c_begin >> 6) + tid; t < ((c_end + 63) >> 6); t += 256) any |= mask[t].x | mask[t].y;
    if (!__syncthreads_or((int)(any != 0)) || (pm.x | pm.y) == 0) return;
  }
  const int rowbase = wave * 16;
  const int r = lane & 15, qd = lane >> 4;
  // rows rowbase + 4 * qd + e: their ids, and whether they can have a hit at all (live and allowed)
  unsigned qi[4];
  bool rowok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    qi[e] = (unsigned)(i0 + rowbase + 4 * qd + e);
    rowok[e] = true;
    if constexpr (MASKED) rowok[e] = ((((const uint32_t*)mask)[qi[e] >> 5] >> (qi[e] & 31)) & 1u) != 0;
  }
  // Staging as in kernels/knn.hip, for both operands: thread -> (rows tid / 16 + 16 p, p < 4; k step tid % 16),
  // one raw_t = the four k slots of one step; the next slab's loads are issued before this slab's MFMAs.
  const int srow = tid >> 4, sj = tid & 15;
  auto loadg = [&](raw_t(&v)[4], const GT* const(&src)[4], int k0) {
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = k0 + sj * 4 < E ? gal_raw(src[p] + k0) : raw_t{};  // zero bits widen to 0.f
  };
  auto put = [&](float* dst, const raw_t(&v)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float4 wd = gal_widen<GT>(v[p]);
      float* d = dst + (p * 16 + srow) * LDT + sj;
      d[0] = wd.x; d[KQ] = wd.y; d[2 * KQ] = wd.z; d[3 * KQ] = wd.w;
    }
  };
  const GT* pa[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pa[p] = gal + (long)min((unsigned)(i0 + p * 16 + srow), (unsigned)N - 1) * E + sj * 4;
  for (unsigned j0 = c_begin; j0 < c_end; j0 += TB) {
    // A tile whose columns are all at or below the panel's first row has no pair (block-uniform, before any load
    // or barrier).  A guard only: the cut above starts every span at or after the panel's own tile and leaves out
    // the one-row last panel, so no enumerated tile meets it.
    if (j0 + (TB - 1) <= (unsigned)i0) continue;
    uint2 mw = make_uint2(0, 0);  // the tile's allowed bits: columns j0 .. j0 + 31 | j0 + 32 .. j0 + 63
    if constexpr (MASKED) {
      mw = mask[j0 >> 6];
      if ((mw.x | mw.y) == 0) continue;  // block-uniform too
    }
    const GT* pb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) pb[p] = gal + (long)min(j0 + p * 16 + srow, (unsigned)N - 1) * E + sj * 4;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    raw_t va[4], vb[4];
    loadg(va, pa, 0);
    loadg(vb, pb, 0);
    for (int k0 = 0; k0 < E; k0 += TK) {
      __syncthreads();
      put(stage[0], va);
      put(stage[1], vb);
      __syncthreads();
      if (k0 + TK < E) {
        loadg(va, pa, k0 + TK);
        loadg(vb, pb, k0 + TK);
      }
      const int steps = min(TK, E - k0) / 4;  // a multiple of 4 (E % 16 == 0): the last slab may be short
#pragma unroll
      for (int jq = 0; jq < 4; ++jq) {
        if (jq * 4 >= steps) break;
        // 16x16x4: lane (r, qd) supplies A[r][qd] and B[qd][r]; k = k0 + 4 * (4 jq + st) + qd, ascending
        const f32x4 a = *(const f32x4*)&stage[0][(rowbase + r) * LDT + qd * KQ + jq * 4];
        f32x4 bf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) bf[t] = *(const f32x4*)&stage[1][(t * 16 + r) * LDT + qd * KQ + jq * 4];
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st], bf[t][st], acc[t], 0, 0, 0);
      }
    }
    // C[row = 4 * qd + e][col = r] of column tile t; hit bit 4 * e + t.  col < c_end <= N and col > row: both < N
    unsigned hit = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned col = j0 + t * 16 + r;
        bool ok = col < c_end && col > qi[e] && rowok[e];
        if constexpr (MASKED) ok = ok && (((t < 2 ? mw.x : mw.y) >> ((t & 1) * 16 + r)) & 1u) != 0;
        if (ok && fmaf(acc[t][e], scale, bias) >= thr) hit |= 1u << (4 * e + t);
      }
    if (__ballot(hit != 0) == 0) continue;  // wave-uniform: the common case
    if (hit != 0) {
      // parent[] once per row and column of this lane that has a hit; equal entries: the same tree already
      int pr[4], pc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) pr[e] = ((hit >> (4 * e)) & 0xfu) ? uf_load(parent, qi[e]) : -1;
#pragma unroll
      for (int t = 0; t < 4; ++t) pc[t] = (hit & (0x1111u << t)) ? uf_load(parent, j0 + t * 16 + r) : -2;
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (((hit >> (4 * e + t)) & 1u) && pr[e] != pc[t]) uf_unite(parent, (int)qi[e], (int)(j0 + t * 16 + r));
    }
  }
}

template <bool MASKED>
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, int N, const uint32_t* __restrict__ mask,
                                                         int* __restrict__ label, uint32_t* __restrict__ groups,
                                                         unsigned* __restrict__ count) {
  // whole waves walk the slots, so that the ballot below has every lane
  for (long base = ((long)blockIdx.x * 256 + (threadIdx.x & ~63)); base < N; base += (long)gridDim.x * 256) {
    const long i = base + (threadIdx.x & 63);
    bool ok = i < N;
    if constexpr (MASKED)
      if (ok) ok = ((mask[i >> 5] >> (i & 31)) & 1u) != 0;
    const int l = ok ? uf_find(parent, (int)i) : -1;
    if (i < N) {
      if (label) label[i] = l;
      if (groups) groups[i] = ok ? (uint32_t)l : (kUngrouped | (uint32_t)i);
    }
    const uint64_t roots = __ballot(ok && l == (int)i);
    if (count && (threadIdx.x & 63) == 0 && roots != 0) atomicAdd(count, (unsigned)__popcll(roots));
  }
}

CcCut cc_cut(int N) {
  CcCut c;
  c.n_tiles = (N + TB - 1) / TB;
  const long tri = (long)c.n_tiles * (c.n_tiles + 1) / 2;
  long T = std::min<long>(kCcSpanTiles, std::max(1L, (tri + kCcBlocks - 1) / kCcBlocks));
  const long forced = g_topk_span_cols.load();
  if (forced > 0) T = std::max(1L, forced / TB);
  T = std::max(T, (tri + (1L << 29) - 1) >> 29);  // the grid stays below 2^31 blocks (T / 2 tiles at least, but for the T tail blocks)
  c.T = (int)std::min<long>(T, c.n_tiles);
  const long M = (c.n_tiles - 1) / c.T;  // the last group, of n_tiles - M T panels with M + 1 spans each
  c.first = (N - 1) % TB == 0 ? 1 : 0;   // the last panel is row N - 1 alone: no column above it
  c.blocks = (long)c.T * M * (M + 1) / 2 + (c.n_tiles - M * c.T) * (M + 1) - c.first;
  return c;
}

template <typename GT, bool MASKED>
void launch_cc_join(const ComponentsArgs& a, const CcCut& c) {
  hipLaunchKernelGGL((cc_join_kernel<GT, MASKED>), dim3((unsigned)c.blocks), dim3(256), 0, a.stream, (const GT*)a.g, a.N,
                     a.E, a.scale, a.bias, a.threshold, c, (const uint2*)a.mask, a.parent);
}

// Every instantiation: [gallery type][MASKED].
typedef void (*CcJoin)(const ComponentsArgs&, const CcCut&);
#define CC_GT(GT) { launch_cc_join<GT, false>, launch_cc_join<GT, true> }
constexpr CcJoin kCcJoin[3][2] = {CC_GT(float), CC_GT(_Float16), CC_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kCcJoin");

}  // namespace

hipError_t launch_components(const ComponentsArgs& a) {
  if (a.N < 0 || a.E <= 0 || a.E % 16 != 0 || a.threshold != a.threshold) return hipErrorInvalidValue;
  if (a.N > 0 && (!a.g || !a.parent || (!a.label && !a.groups))) return hipErrorInvalidValue;
  if (a.mask && ((uintptr_t)a.mask & 7)) return hipErrorInvalidValue;
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  const int row_blocks = (int)std::min<long>(std::max(1L, ((long)a.N + 255) / 256), 4096);
  hipLaunchKernelGGL(cc_init_kernel, dim3(row_blocks), dim3(256), 0, a.stream, a.parent, a.N, a.count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.N == 0) return e;
  const CcCut c = cc_cut(a.N);
  if (c.blocks > INT32_MAX) return hipErrorInvalidValue;
  if (c.blocks > 0) {  // N == 1 has no pair
    kCcJoin[a.dtype][a.mask != nullptr](a, c);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.mask)
    hipLaunchKernelGGL(cc_flatten_kernel<true>, dim3(row_blocks), dim3(256), 0, a.stream, a.parent, a.N, a.mask, a.label,
                       a.groups, a.count);
  else
    hipLaunchKernelGGL(cc_flatten_kernel<false>, dim3(row_blocks), dim3(256), 0, a.stream, a.parent, a.N, a.mask, a.label,
                       a.groups, a.count);
  return hipGetLastError();
}

}  // namespace clipgpu
