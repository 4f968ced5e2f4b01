// Inverted lists of the embedding index (clipgpu_index_partition): the rows grouped by their assignment label,
// in CSR form -- offsets [C + 1] and ids [n_live], the ids of a list ascending.  Not a hot path: it runs once
// per partition, after the assignment, which costs a thousand times more.
//
// The CSR must be a pure function of the labels, the same bits on every run, so no atomic decides where an id
// goes.  It is a stable LSD counting sort of the row ids by label in 8-bit digits: one pass for C <= 256, two
// up to 65,536.  A pass over n items, cut into chunks of kChunk consecutive items, one one-wave block each:
//
//   histogram  hist[chunk][digit] = the chunk's valid items with that digit   (LDS counters: a count does not
//              depend on the order of its increments)
//   scan       hist[chunk][digit] <- the items with a smaller digit + the items with this digit in earlier
//              chunks: where the chunk's first item with that digit goes          (one block, digit per thread)
//   scatter    the chunk again, 64 items at a time in order: a lane's rank among the lanes with its digit comes
//              from eight ballots (one per bit of the digit), the running start of each digit is in LDS
//
// so equal digits keep their order: pass 1 orders the live rows (ascending to begin with) by the low byte of
// the label, pass 2 by the high byte.  offsets is the exclusive scan of the histogram of the labels (global
// integer counters, for the same reason order-free).  A label outside [0, C) marks a row that is in no list.
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"
#include "topk_stage.hpp"

namespace clipgpu {

namespace {

constexpr int kChunk = 1024;  // items per block of a pass: 16 rounds of one wave
constexpr int kDigits = 256;
inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
inline long chunks_of(long N) { return (N + kChunk - 1) / kChunk; }

__global__ __launch_bounds__(256) void lists_count_kernel(const int32_t* __restrict__ label, int N, int C,
                                                          int* __restrict__ count) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const int l = label[i];
    if ((unsigned)l < (unsigned)C) atomicAdd(&count[l], 1);
  }
}

// offsets[c] = count[0] + ... + count[c - 1] for c <= C.  One block: a thread sums a run of ceil(C / 256)
// counts, thread 0 scans the 256 sums, every thread writes its run.
__global__ __launch_bounds__(256) void lists_offsets_kernel(const int* __restrict__ count, int C,
                                                            int32_t* __restrict__ offsets) {
  __shared__ int part[256];
  const int t = threadIdx.x, run = (C + 255) / 256;
  const int c0 = min(t * run, C), c1 = min(c0 + run, C);
  int sum = 0;
  for (int c = c0; c < c1; ++c) sum += count[c];
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int i = 0; i < 256; ++i) {
      const int v = part[i];
      part[i] = acc;
      acc += v;
    }
    offsets[C] = acc;
  }
  __syncthreads();
  int at = part[t];
  for (int c = c0; c < c1; ++c) {
    offsets[c] = at;
    at += count[c];
  }
}

// Item i of a pass: FIRST -- row i (valid if its label is in [0, C)), digit = the label's low byte; else --
// in[i] for i < *n_items, digit = the high byte of that row's label.  Returns the row, or -1.
template <bool FIRST>
__device__ __forceinline__ int pass_item(long i, const int32_t* label, int N, int C, const int32_t* in,
                                         const int32_t* n_items, int& digit) {
  int row = -1;
  digit = 0;
  if (FIRST) {
    if (i < N) {
      const int l = label[i];
      if ((unsigned)l < (unsigned)C) {
        row = (int)i;
        digit = l & 255;
      }
    }
  } else if (i < *n_items) {
    row = in[i];
    digit = (label[row] >> 8) & 255;
  }
  return row;
}

template <bool FIRST>
__global__ __launch_bounds__(64) void lists_hist_kernel(const int32_t* __restrict__ label, int N, int C,
                                                        const int32_t* __restrict__ in,
                                                        const int32_t* __restrict__ n_items, int* __restrict__ hist) {
  __shared__ int h[kDigits];
  const int lane = threadIdx.x;
  for (int d = lane; d < kDigits; d += 64) h[d] = 0;
  wave_lds_order();
  const long first = (long)blockIdx.x * kChunk;
  for (int round = 0; round < kChunk / 64; ++round) {
    int digit;
    const int row = pass_item<FIRST>(first + round * 64 + lane, label, N, C, in, n_items, digit);
    if (row >= 0) atomicAdd(&h[digit], 1);
  }
  wave_lds_order();
  for (int d = lane; d < kDigits; d += 64) hist[(long)blockIdx.x * kDigits + d] = h[d];
}

// hist[chunk][digit] (counts) -> where the chunk's first item with that digit goes.  One block, thread = digit.
__global__ __launch_bounds__(kDigits) void lists_scan_kernel(int* __restrict__ hist, int chunks) {
  __shared__ int total[kDigits];
  const int d = threadIdx.x;
  int run = 0;
  for (long b = 0; b < chunks; ++b) {
    const int v = hist[b * kDigits + d];
    hist[b * kDigits + d] = run;
    run += v;
  }
  total[d] = run;
  __syncthreads();
  if (d == 0) {
    int acc = 0;
    for (int i = 0; i < kDigits; ++i) {
      const int v = total[i];
      total[i] = acc;
      acc += v;
    }
  }
  __syncthreads();
  const int base = total[d];
  for (long b = 0; b < chunks; ++b) hist[b * kDigits + d] += base;
}

template <bool FIRST>
__global__ __launch_bounds__(64) void lists_scatter_kernel(const int32_t* __restrict__ label, int N, int C,
                                                           const int32_t* __restrict__ in,
                                                           const int32_t* __restrict__ n_items,
                                                           const int* __restrict__ hist, int32_t* __restrict__ out) {
  __shared__ int at[kDigits];  // where the next item of each digit goes
  const int lane = threadIdx.x;
  for (int d = lane; d < kDigits; d += 64) at[d] = hist[(long)blockIdx.x * kDigits + d];
  wave_lds_order();
  const long first = (long)blockIdx.x * kChunk;
  for (int round = 0; round < kChunk / 64; ++round) {
    int digit;
    const int row = pass_item<FIRST>(first + round * 64 + lane, label, N, C, in, n_items, digit);
    const bool valid = row >= 0;
    uint64_t peers = __ballot(valid);  // the valid lanes with this lane's digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = ((digit >> bit) & 1) != 0;
      const uint64_t m = __ballot(one);
      peers &= one ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    // at most N valid items in all, so the position lies below N (pass 1) or *n_items (pass 2)
    if (valid) out[at[digit] + rank] = row;
    wave_lds_order();
    if (valid && rank == 0) at[digit] += __popcll(peers);
    wave_lds_order();
  }
}

struct ListsTmp { int* count; int* hist; int32_t* ids; };
ListsTmp carve_tmp(void* tmp, long N) {
  char* p = (char*)tmp;
  ListsTmp t;
  t.count = (int*)p;
  p += align256((size_t)kClusterMaxCentroids * 4);
  t.hist = (int*)p;
  p += align256((size_t)chunks_of(N) * kDigits * 4);
  t.ids = (int32_t*)p;
  return t;
}

}  // namespace

size_t lists_tmp_bytes(long N) {
  return align256((size_t)kClusterMaxCentroids * 4) + align256((size_t)chunks_of(N) * kDigits * 4) + align256((size_t)N * 4);
}

hipError_t launch_lists(const int32_t* label, int N, int C, int32_t* offsets, int32_t* ids, void* tmp, hipStream_t s) {
  if (!label || !offsets || !ids || !tmp || N <= 0 || C < 1 || C > kClusterMaxCentroids) return hipErrorInvalidValue;
  const ListsTmp t = carve_tmp(tmp, N);
  const int chunks = (int)chunks_of(N);
  hipError_t err = hipMemsetAsync(t.count, 0, (size_t)C * 4, s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(lists_count_kernel, dim3((int)std::min<long>(((long)N + 255) / 256, 1024)), dim3(256), 0, s, label, N,
                     C, t.count);
  hipLaunchKernelGGL(lists_offsets_kernel, dim3(1), dim3(256), 0, s, t.count, C, offsets);
  const bool two = C > kDigits;
  int32_t* first_out = two ? t.ids : ids;
  hipLaunchKernelGGL(lists_hist_kernel<true>, dim3(chunks), dim3(64), 0, s, label, N, C, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, t.hist);
  hipLaunchKernelGGL(lists_scan_kernel, dim3(1), dim3(kDigits), 0, s, t.hist, chunks);
  hipLaunchKernelGGL(lists_scatter_kernel<true>, dim3(chunks), dim3(64), 0, s, label, N, C, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, t.hist, first_out);
  if (two) {  // the items are now the live rows: offsets[C] of them, which only the device knows
    hipLaunchKernelGGL(lists_hist_kernel<false>, dim3(chunks), dim3(64), 0, s, label, N, C, (const int32_t*)t.ids,
                       (const int32_t*)(offsets + C), t.hist);
    hipLaunchKernelGGL(lists_scan_kernel, dim3(1), dim3(kDigits), 0, s, t.hist, chunks);
    hipLaunchKernelGGL(lists_scatter_kernel<false>, dim3(chunks), dim3(64), 0, s, label, N, C, (const int32_t*)t.ids,
                       (const int32_t*)(offsets + C), t.hist, ids);
  }
  return hipGetLastError();
}

}  // namespace clipgpu
