// Storage conversion of the embedding index's gallery (csrc/index.hip): f32 rows to the gallery's element
// type on their way in -- appended (gal_round_kernel) or scattered to given row ids (gal_scatter_kernel) --
// and back to f32 on their way out (gal_widen_kernel).  f32 -> f16 / bf16 rounds to nearest even (round16);
// 16 bits -> f32 is exact (gal4, gallery.hpp, which the search kernels of topk.hip read the gallery with).
// A thread moves four elements per step: a 16-byte f32 access against an 8-byte one of the 16-bit side.
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "gallery.hpp"
#include "kernels.hpp"

namespace clipgpu {

namespace {

__device__ __forceinline__ uint32_t round16(float x, _Float16*) {
  const _Float16 h = (_Float16)x;  // v_cvt_f16_f32: nearest even, subnormals kept, |x| >= 65520 -> inf
  return (uint32_t) __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ uint32_t round16(float x, __bf16*) {
  const uint32_t b = __float_as_uint(x);
  if ((b & 0x7fffffffu) > 0x7f800000u) return (b >> 16) | 0x40u;  // NaN stays NaN (quiet), sign kept
  return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;                    // carries into the exponent, up to inf
}

// Four f32 values to elements 4 * i4 .. 4 * i4 + 3 of a gallery: rounded and packed for a 16-bit one, the
// bits themselves for an f32 one.
__device__ __forceinline__ void gal_store4(float* out, long i4, float4 v) { ((float4*)out)[i4] = v; }
template <typename GT> __device__ __forceinline__ void gal_store4(GT* out, long i4, float4 v) {
  uint2 o;
  o.x = round16(v.x, (GT*)nullptr) | (round16(v.y, (GT*)nullptr) << 16);
  o.y = round16(v.z, (GT*)nullptr) | (round16(v.w, (GT*)nullptr) << 16);
  ((uint2*)out)[i4] = o;
}

// The packing is written out here too: through gal_store4 the bf16 instantiation compiles to another order.
template <typename GT>
__global__ __launch_bounds__(256) void gal_round_kernel(const float* __restrict__ in, GT* __restrict__ out, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 v = ((const float4*)in)[i];
    uint2 o;
    o.x = round16(v.x, (GT*)nullptr) | (round16(v.y, (GT*)nullptr) << 16);
    o.y = round16(v.z, (GT*)nullptr) | (round16(v.w, (GT*)nullptr) << 16);
    ((uint2*)out)[i] = o;
  }
}

template <typename GT>
__global__ __launch_bounds__(256) void gal_widen_kernel(const GT* __restrict__ in, float* __restrict__ out, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256)
    ((float4*)out)[i] = gal4(in + 4 * i);
}

// Row i of `in` (f32 [n][E]) to row ids[i] of the gallery, rounded as gal_round_kernel rounds (an f32
// gallery takes the bits).  The ids are distinct and inside the gallery (checked by the caller).
template <typename GT>
__global__ __launch_bounds__(256) void gal_scatter_kernel(const float* __restrict__ in, const int64_t* __restrict__ ids,
                                                          GT* __restrict__ gal, long n, int E4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n * E4; i += (long)gridDim.x * 256) {
    const long row = i / E4, c = i - row * E4;
    gal_store4(gal, ids[row] * E4 + c, ((const float4*)in)[i]);
  }
}

int convert_blocks(long n4) { return (int)std::min<long>((n4 + 255) / 256, 8192); }

}  // namespace

int topk_gal_bytes(int dtype) { return dtype == TOPK_GAL_F32 ? 4 : 2; }

hipError_t launch_gal_round(int dtype, const float* in, void* out, long n, hipStream_t s) {
  if (n <= 0 || n % 4 || (dtype != TOPK_GAL_F16 && dtype != TOPK_GAL_BF16)) return hipErrorInvalidValue;
  const dim3 grid(convert_blocks(n / 4));
  if (dtype == TOPK_GAL_F16) hipLaunchKernelGGL(gal_round_kernel<_Float16>, grid, dim3(256), 0, s, in, (_Float16*)out, n / 4);
  else hipLaunchKernelGGL(gal_round_kernel<__bf16>, grid, dim3(256), 0, s, in, (__bf16*)out, n / 4);
  return hipGetLastError();
}

hipError_t launch_gal_widen(int dtype, const void* in, float* out, long n, hipStream_t s) {
  if (n <= 0 || n % 4 || (dtype != TOPK_GAL_F16 && dtype != TOPK_GAL_BF16)) return hipErrorInvalidValue;
  const dim3 grid(convert_blocks(n / 4));
  if (dtype == TOPK_GAL_F16) hipLaunchKernelGGL(gal_widen_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)in, out, n / 4);
  else hipLaunchKernelGGL(gal_widen_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)in, out, n / 4);
  return hipGetLastError();
}

hipError_t launch_gal_scatter(int dtype, const float* in, const int64_t* ids, void* gal, long n, int E, hipStream_t s) {
  if (n <= 0 || E <= 0 || E % 4) return hipErrorInvalidValue;
  const int blocks = convert_blocks(n * (E / 4));
  if (dtype == TOPK_GAL_F32)
    hipLaunchKernelGGL(gal_scatter_kernel<float>, dim3(blocks), dim3(256), 0, s, in, ids, (float*)gal, n, E / 4);
  else if (dtype == TOPK_GAL_F16)
    hipLaunchKernelGGL(gal_scatter_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, in, ids, (_Float16*)gal, n, E / 4);
  else if (dtype == TOPK_GAL_BF16)
    hipLaunchKernelGGL(gal_scatter_kernel<__bf16>, dim3(blocks), dim3(256), 0, s, in, ids, (__bf16*)gal, n, E / 4);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace clipgpu
