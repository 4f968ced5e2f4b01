// Device-side reading of a 16-bit gallery row, shared by the search (kernels/topk.hip) and the storage
// conversion (kernels/gallery.hip).
#pragma once
#include "common.hpp"

namespace clipgpu {

// Four consecutive 16-bit gallery elements as f32: one 8-byte load, widened (exactly).
__device__ __forceinline__ float4 gal4(const _Float16* p) {
  const f16x4 h = *(const f16x4*)p;
  return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}
__device__ __forceinline__ float4 gal4(const __bf16* p) {
  const uint2 u = *(const uint2*)p;
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}

}  // namespace clipgpu
