// Integer scans over a table of ids, shared by the kernels that turn "marked entries of a [V] table" into ranks in increasing
// id (csrc/sample.hip: the new nodes of a hop; csrc/triple_batch.hip: the distinct endpoints of a triple batch).
// A workgroup is 256 threads (4 waves of 64) and owns chunks of 1024 ids, 4 per thread.
#pragma once
#include "common.hpp"

namespace tfgnn {

constexpr int kScanThreads = 256;
constexpr int kScanChunk = 1024;  // rows (or ids) whose counts one workgroup scans: 4 per thread

// exclusive scan of one value per thread over the workgroup (4 waves of 64); *total: the workgroup's sum
__device__ __forceinline__ int32_t block_exclusive_scan(int32_t x, int32_t* total, int32_t* wave_sums) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wave_sums[w] = incl;
  __syncthreads();
  int32_t base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kScanThreads / 64; ++k) {
    const int32_t s = wave_sums[k];
    if (k < w) base += s;
    tot += s;
  }
  __syncthreads();  // wave_sums may be written again
  *total = tot;
  return base + incl - x;
}

// ONE workgroup: the chunk totals off[0 : chunks] -> their exclusive offsets, in place, with a carry across rounds of 256
// chunks; returns the grand total (the same value in every thread).  off[chunks] is not touched.
__device__ __forceinline__ int32_t scan_chunk_totals(int32_t* off, int64_t chunks, int32_t* wave_sums) {
  int32_t carry = 0;
  for (int64_t c0 = 0; c0 < chunks; c0 += kScanThreads) {
    const int64_t ck = c0 + threadIdx.x;
    const int32_t x = ck < chunks ? off[ck] : 0;
    int32_t total;
    const int32_t ex = block_exclusive_scan(x, &total, wave_sums);
    if (ck < chunks) off[ck] = carry + ex;
    carry += total;
  }
  return carry;
}

// the workgroups of a grid, chunk by chunk: counts[ck] = the number of ids v in chunk ck of [0, V) with table[v] == mark
__device__ __forceinline__ void count_marked_chunks(const int32_t* table, int32_t V, int32_t mark, int32_t* counts,
                                                    int32_t* wave_sums) {
  const int64_t chunks = ((int64_t)V + kScanChunk - 1) / kScanChunk;
  for (int64_t ck = blockIdx.x; ck < chunks; ck += gridDim.x) {
    int32_t n = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t v = ck * kScanChunk + q * kScanThreads + threadIdx.x;
      if (v < V && table[v] == mark) ++n;
    }
    int32_t total;
    block_exclusive_scan(n, &total, wave_sums);
    if (threadIdx.x == 0) counts[ck] = total;
  }
}

// the workgroups of a grid, chunk by chunk: the marked ids take the ranks first + counts_scanned[ck] + (rank inside the
// chunk), increasing with the id (thread x owns ids 4 x .. 4 x + 3 of its chunk).  A rank below `capacity`: table[v] = rank
// and out[rank] = v; a rank at or beyond it: table[v] = -1 (it is in no output, so a restore pass would not find it).
__device__ __forceinline__ void assign_marked_chunks(int32_t* table, int32_t V, int32_t mark, const int32_t* counts_scanned,
                                                     int32_t first, int32_t capacity, int32_t* out, int32_t* wave_sums) {
  const int64_t chunks = ((int64_t)V + kScanChunk - 1) / kScanChunk;
  for (int64_t ck = blockIdx.x; ck < chunks; ck += gridDim.x) {
    const int64_t v0 = ck * kScanChunk + threadIdx.x * 4;
    bool m[4];
    int32_t n = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      m[q] = v0 + q < V && table[v0 + q] == mark;
      n += m[q];
    }
    int32_t total;
    int32_t rank = block_exclusive_scan(n, &total, wave_sums);
    if (total == 0) continue;
    const int64_t base = (int64_t)first + counts_scanned[ck];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!m[q]) continue;
      const int64_t id = base + rank++;
      if (id < capacity) {
        table[v0 + q] = (int32_t)id;
        out[id] = (int32_t)(v0 + q);
      } else {
        table[v0 + q] = -1;
      }
    }
  }
}

static inline unsigned scan_strided_grid(int64_t items, int64_t per_block, int64_t max_blocks) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, per_block), max_blocks));
}

}  // namespace tfgnn
