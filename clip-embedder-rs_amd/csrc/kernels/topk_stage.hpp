// What the phase-1 kernels of the embedding index share (kernels/topk.hip: the k best; kernels/range.hip:
// every row at or above a threshold): the tile sizes, the [row][k slot][k step] staging layout that fixes
// the k order of the v_mfma_f32_16x16x4_f32 chain -- and with it the bits of a score -- and the gallery
// element as loaded and as staged.
#pragma once
#include "common.hpp"
#include "gallery.hpp"

namespace clipgpu {

constexpr int TB = 64, TK = 64;
constexpr int KQ = 20, LDT = 88;  // staged row: 4 k slots of 16 steps + 4, + 8: conflict-free 16-byte reads
constexpr int NB = 16;            // the few-query kernels' tile: 16 query rows x 16 columns, one wave

// LDS traffic of one wave is processed in program order; this keeps the compiler from moving it.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The same elements as loaded (held in registers while the loads are in flight) and widened when staged.
template <typename GT> struct GalRaw { typedef uint2 type; };
template <> struct GalRaw<float> { typedef float4 type; };
__device__ __forceinline__ float4 gal_raw(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ uint2 gal_raw(const _Float16* p) { return *(const uint2*)p; }
__device__ __forceinline__ uint2 gal_raw(const __bf16* p) { return *(const uint2*)p; }
template <typename GT> __device__ __forceinline__ float4 gal_widen(float4 v) { return v; }
template <typename GT> __device__ __forceinline__ float4 gal_widen(uint2 u) {
  union { uint2 u; GT h[4]; } x;
  x.u = u;
  return gal4(x.h);
}

}  // namespace clipgpu
