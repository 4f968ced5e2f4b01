// Probed (IVF) phase 1 of the embedding index (clipgpu_index_search_probed): the few-query kernel of topk.hip
// with two indirections.  The gallery is partitioned into inverted lists (kernels/lists.hip: ids [n_live] in
// CSR form, offsets [C + 1]); a coarse search of the C centroids (launch_topk over the centroids as a gallery)
// has chosen n_probe lists per query.  Here a block is ONE wave that owns (query q, probe p, part s):
//
//   list  = coarse[q][p]
//   tiles = [s * T, (s + 1) * T) of the list's ceil(len / 16) 16-row tiles, T = ceil(tiles / parts)
//   row   = ids[pos] where the few-query kernel has its column;  key = topk_key(score bits, ids[pos]);
//   bit   = mask[id >> 5] >> (id & 31)  (MASKED)
//
// and writes its k best to ws[((q * n_probe + p) * parts + s) * k ..] for topk_merge_kernel (n_spans =
// n_probe * parts), or k empty entries when its tile range or its list is empty.  Keys carry the row id, and a
// row is in one list only, so keys are unique over everything the merge sees: the result does not depend on
// the lists, the parts or the order rows are met in.
//
// What is shared with topk_narrow_kernel, unchanged: the [k slot][k step] staging of topk_stage.hpp and the
// v_mfma_f32_16x16x4_f32 chain in the same k order (the bits of a score are similarity's), compact_row
// (topk_select.hpp), and the flat request sequence over (tile, slab), two slabs ahead, every request the same
// loads whatever the position (topk.hip explains what a conditional load does to the counting of the loads in
// flight).  Row 0 of the 16-row query tile is the query; it is the only row of the accumulator that is read.
// The query side therefore stages rows 0 .. 3 only (one load, the same row four times: a lane stages the row
// lane / 16) and the rest of the A tile stays zero.
//
// The ids.  A request's row loads need the ids of its tile in registers, so they are fetched ahead: every
// request also loads the ids of the tile that the NEXT request on the same register set (two requests on) will
// read -- four per lane in the staging layout (rows lane / 16 + 4 p) and one in the accumulator layout (column
// lane % 16, for the key and the mask bit) -- and by the time that request is made they have arrived with the
// slab that was staged just before it.  Only the first two requests wait for ids they asked for themselves.
// MASKED: the request loads the word of its column's id, which is in a register by then, so the selection
// starts no load.  Positions past the end of the block's range are clamped for the loads (the range is not
// empty) and kept out of the selection; ids are clamped below N before they address the gallery or the mask.
#include <cstdint>

#include "common.hpp"
#include "gallery.hpp"
#include "kernels.hpp"
#include "topk_key.hpp"
#include "topk_select.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

// KC: list capacity the LDS is sized for (k <= KC).  LDS: 11 KiB of staging + (KC + 32) entries.
template <int KC, typename GT, bool MASKED>
__global__ __launch_bounds__(64) void topk_probe_kernel(const float* __restrict__ qry, const GT* __restrict__ gal, int N,
                                                        int E, float scale, float bias, int k,
                                                        const int64_t* __restrict__ coarse, int n_probe, int parts,
                                                        const int32_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ ids,
                                                        const uint32_t* __restrict__ mask, uint2* __restrict__ ws) {
  typedef typename GalRaw<GT>::type raw_t;
  constexpr int STRIDE = KC + CAND1;
  __shared__ __attribute__((aligned(16))) float stage[2][NB * LDT];  // A | B: [row][k slot qd][k step]
  __shared__ uint2 sel[STRIDE];
  const int lane = threadIdx.x;
  const int q = blockIdx.y, p = blockIdx.x / parts, s = blockIdx.x - p * parts;
  uint2* dst = ws + (((long)q * n_probe + p) * parts + s) * k;
  const long list = coarse[(long)q * n_probe + p];
  unsigned pos_begin = 0, pos_end = 0;  // the block's positions in ids; unsigned as the few-query kernel's columns
  if (list >= 0) {
    const unsigned beg = (unsigned)offsets[list], end = (unsigned)offsets[list + 1];
    const unsigned tiles = (end - beg + NB - 1) / NB, T = (tiles + parts - 1) / parts;
    const unsigned t0 = min((unsigned)s * T, tiles), t1 = min(t0 + T, tiles);
    pos_begin = beg + t0 * NB;
    pos_end = t1 == tiles ? end : beg + t1 * NB;
  }
  if (pos_begin >= pos_end) {  // block-uniform: no list, an empty list or a part past its tiles
    for (int t = lane; t < k; t += 64) dst[t] = ent_empty();
    return;
  }
  for (int i = lane; i < STRIDE; i += 64) sel[i] = ent_empty();
  for (int i = lane; i < NB * LDT; i += 64) stage[0][i] = 0.f;  // query rows 4 .. 15 stay zero
  wave_lds_order();
  const int r = lane & 15, qd = lane >> 4;
  const int srow = lane >> 4, sj = lane & 15;  // staging as in the few-query kernel: rows srow + 4 p, k step sj
  const float* pa = qry + (long)q * E;
  const unsigned last = pos_end - 1, nmax = (unsigned)N - 1;
  uint64_t thr = 0;  // the threshold of the query's list, and its candidates: wave-uniform
  int c = 0;
  unsigned rj = pos_begin, aj = pos_begin;  // the next slab to request: tile rj, k rk; (aj, ak): two requests on
  int rk = 0, ak = 0;
  auto advance = [&](unsigned& j, int& kk) {
    kk += TK;
    if (kk >= E) {
      kk = 0;
      j += NB;
    }
  };
  auto load_ids = [&](unsigned j, int(&vi)[4], int& vs) {
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) vi[pp] = ids[min(j + pp * 4 + srow, last)];
    vs = ids[min(j + r, last)];
  };
  // One request: the mask word (MASKED), one query load, four row loads, five id loads -- the same loads
  // whatever the position.  vi / vs come in as the ids of this request's tile and go out as the loads of the
  // ids of the tile two requests on; su keeps this tile's column id for the step that stages the slab.
  auto request = [&](float4& va, raw_t(&vb)[4], int(&vi)[4], int& vs, int& su, uint32_t& vm) {
    const int ko = min(rk + sj * 4, E - 4);
    su = vs;
    if constexpr (MASKED) vm = mask[min((unsigned)su, nmax) >> 5];
    va = *(const float4*)(pa + ko);
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) vb[pp] = gal_raw(gal + (long)min((unsigned)vi[pp], nmax) * E + ko);
    load_ids(aj, vi, vs);
    advance(rj, rk);
    advance(aj, ak);
  };
  auto put = [&](float* d0, int pp, float4 v) {
    float* d = d0 + (pp * 4 + srow) * LDT + sj;
    d[0] = v.x; d[KQ] = v.y; d[2 * KQ] = v.z; d[3 * KQ] = v.w;
  };
  // C[row 0][col = r] of the tile at position cj, in the lanes qd == 0: the merge kernel's selection on one list.
  auto select = [&](unsigned cj, const f32x4& acc, int sid, bool allowed) {
    const uint32_t bits = __float_as_uint(fmaf(acc[0], scale, bias));
    const uint64_t key = topk_key(bits, (uint32_t)sid);
    const bool live = qd == 0 && cj + r <= last && allowed;
    bool pass = live && key > thr;
    uint64_t bal = __ballot(pass);
    if (bal == 0) return;  // wave-uniform: the common case once the threshold has warmed up
    if (c + __popcll(bal) > CAND1) {
      thr = compact_row(sel, k, c, lane);
      c = 0;
      pass = live && key > thr;
      bal = __ballot(pass);
    }
    if (pass) sel[k + c + __popcll(bal & ((1ull << lane) - 1ull))] = make_uint2(bits, (uint32_t)sid);
    wave_lds_order();
    c += __popcll(bal);
  };
  unsigned cj = pos_begin;  // the slab in hand: tile cj, k ck
  int ck = 0;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step = [&](float4& va, raw_t(&vb)[4], int(&vi)[4], int& vs, int& su, uint32_t& vm) {
    put(stage[0], 0, va);
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) put(stage[1], pp, gal_widen<GT>(vb[pp]));
    // this slab's column id and its bit, taken before the request below reuses the registers
    const int sid = su;
    bool allowed = true;
    if constexpr (MASKED) allowed = ((vm >> (sid & 31)) & 1u) != 0;
    wave_lds_order();
    request(va, vb, vi, vs, su, vm);  // two slabs ahead; the slab after this one is already in flight
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
      select(cj, acc, sid, allowed);
      acc = f32x4{0.f, 0.f, 0.f, 0.f};
      ck = 0;
      cj += NB;
    }
  };
  float4 a0 = {}, a1 = {};
  raw_t b0[4] = {}, b1[4] = {};
  int i0[4], i1[4], s0, s1, u0 = 0, u1 = 0;
  uint32_t m0 = 0, m1 = 0;
  // The ids of the first two requests are loaded here and waited for; (aj, ak) then stands at request 2.
  load_ids(aj, i0, s0);
  advance(aj, ak);
  load_ids(aj, i1, s1);
  advance(aj, ak);
  // The steps run in pairs, a fixed number of them, as in the few-query kernel: an odd count ends in one step
  // past the range, which stages clamped rows and, if it completes a tile, selects nothing (cj > last).
  request(a0, b0, i0, s0, u0, m0);
  __builtin_amdgcn_sched_barrier(0);
  request(a1, b1, i1, s1, u1, m1);
  __builtin_amdgcn_sched_barrier(0);
  const int n_steps = (int)((pos_end - pos_begin + NB - 1) / NB) * ((E + TK - 1) / TK);
  for (int it = 0; it < n_steps; it += 2) {
    step(a0, b0, i0, s0, u0, m0);
    step(a1, b1, i1, s1, u1, m1);
  }
  if (c > 0) compact_row(sel, k, c, lane);
  for (int t = lane; t < k; t += 64) dst[t] = sel[t];
}

template <int KC, typename GT, bool MASKED>
void launch_probe_one(const ProbeArgs& a) {
  hipLaunchKernelGGL((topk_probe_kernel<KC, GT, MASKED>), dim3(a.n_probe * a.parts, a.nq), dim3(64), 0, a.stream, a.q,
                     (const GT*)a.g, a.N, a.E, a.scale, a.bias, a.k, a.coarse, a.n_probe, a.parts, a.offsets, a.ids,
                     a.mask, (uint2*)a.ws);
}

// Every instantiation: [gallery type][MASKED][list capacity 16 / 32 / 64 / 128].
typedef void (*Probe)(const ProbeArgs&);
#define PROBE_KC(GT, M) \
  { launch_probe_one<16, GT, M>, launch_probe_one<32, GT, M>, launch_probe_one<64, GT, M>, launch_probe_one<128, GT, M> }
#define PROBE_GT(GT) \
  { PROBE_KC(GT, false), PROBE_KC(GT, true) }
constexpr Probe kProbe[3][2][4] = {PROBE_GT(float), PROBE_GT(_Float16), PROBE_GT(__bf16)};
static_assert(TOPK_GAL_F32 == 0 && TOPK_GAL_F16 == 1 && TOPK_GAL_BF16 == 2, "the first index of kProbe");

}  // namespace

hipError_t launch_probe(const ProbeArgs& a) {
  if (!a.q || !a.g || !a.coarse || !a.offsets || !a.ids || !a.ws) return hipErrorInvalidValue;
  if (a.nq <= 0 || a.nq > 65535 || a.N <= 0 || a.E <= 0 || a.E % 16 != 0 || a.k < 1 || a.k > kTopkMax)
    return hipErrorInvalidValue;
  if (a.n_probe < 1 || a.parts < 1 || (long)a.n_probe * a.parts > 65535) return hipErrorInvalidValue;
  if (a.dtype != TOPK_GAL_F32 && a.dtype != TOPK_GAL_F16 && a.dtype != TOPK_GAL_BF16) return hipErrorInvalidValue;
  const int kc = a.k <= 16 ? 0 : a.k <= 32 ? 1 : a.k <= 64 ? 2 : 3;
  kProbe[a.dtype][a.mask != nullptr][kc](a);
  return hipGetLastError();
}

}  // namespace clipgpu
