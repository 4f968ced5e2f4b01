// The order of a top-k search (kernels/topk.hip, clipgpu_index_search), for host and device:
// descending score, equal scores by ascending gallery index -- what the reference's stable
// sort_by(partial_cmp) gives on an indexed list (src/clip.rs:134-170).
//
//   key(score, index) = (monotone bits of the score) << 32 | ~index
//
// The search returns the k largest keys, and keys are unique (one per gallery index), so the result
// is deterministic whatever order the candidates are met in.  +0.0 and -0.0 share a key prefix
// (they compare equal); a NaN ranks below -inf (prefix 0; L2-normalised embeddings with finite
// scale / bias never produce one).  Key 0 -- a NaN score at index 0xFFFFFFFF, which no gallery
// has (N < 2^31) -- is the empty slot.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CLIPGPU_HD __host__ __device__ inline
#else
#define CLIPGPU_HD inline
#endif

namespace clipgpu {

constexpr uint32_t kTopkEmptyScore = 0x7fc00000u;  // with kTopkEmptyIndex: key 0
constexpr uint32_t kTopkEmptyIndex = 0xffffffffu;

// f32 bits -> u32 that orders as the floats do: NaN 0 < -inf < ... < -0 == +0 < ... < +inf
CLIPGPU_HD uint32_t topk_mono(uint32_t bits) {
  if ((bits & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (bits == 0x80000000u) bits = 0u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

CLIPGPU_HD uint64_t topk_key(uint32_t score_bits, uint32_t index) {
  return ((uint64_t)topk_mono(score_bits) << 32) | (uint32_t)~index;
}

}  // namespace clipgpu
