// The selection state that the top-k kernels share (kernels/topk.hip: the two phase-1 kernels and the merge;
// kernels/probe.hip: the probed phase 1): a selection entry, the empty entry, and the wave-cooperative
// compaction of a row's best list and its candidates.  Moved here from topk.hip word for word when probe.hip
// became their second user (embedding index, probed search, records the ISA comparison).
#pragma once
#include <stdint.h>

#include "common.hpp"
#include "topk_key.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

constexpr int CAND1 = 32;  // phase 1 candidate slots per row (one ballot adds at most 16 to a row)

// A selection entry: x = the score's own f32 bits, y = gallery index.  Compared by topk_key.
__device__ __forceinline__ uint64_t ent_key(uint2 e) { return topk_key(e.x, e.y); }
__device__ __forceinline__ uint2 ent_empty() { return make_uint2(kTopkEmptyScore, kTopkEmptyIndex); }

// Wave-cooperative (all 64 lanes, uniform arguments).  ent[0 .. k) is the row's current best list,
// ent[k .. k + c) its candidates (k + c <= 192).  Leaves the k best of both in ent[0 .. k), best
// first, and returns the key of ent[k - 1]: the row's new threshold (0 while the list has empty
// slots).  Empty entries all have key 0; the position breaks that tie, so ranks are a permutation.
__device__ __forceinline__ uint64_t compact_row(uint2* ent, int k, int c, int lane) {
  const int m = k + c;
  uint2 mine[3];
  uint64_t mk[3];
  int rank[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int i = lane + 64 * s;
    mine[s] = i < m ? ent[i] : ent_empty();
    mk[s] = ent_key(mine[s]);
    rank[s] = 0;
  }
  for (int j = 0; j < m; ++j) {
    const uint64_t kj = ent_key(ent[j]);  // same address in every lane: an LDS broadcast
#pragma unroll
    for (int s = 0; s < 3; ++s)
      if (64 * s < m) rank[s] += (kj > mk[s] || (kj == mk[s] && j < lane + 64 * s)) ? 1 : 0;
  }
  wave_lds_order();
#pragma unroll
  for (int s = 0; s < 3; ++s)
    if (lane + 64 * s < m && rank[s] < k) ent[rank[s]] = mine[s];
  wave_lds_order();
  return ent_key(ent[k - 1]);
}

}  // namespace clipgpu
