// Dropping a batch's positives from its sampled subgraph (include/tfgnn.h "Excluding a batch's positives"): runs on the
// outputs of tfgnn_neighbor_sample, on the same stream, before anything is read back.
//
// tfgnn_sample_exclude_edges enqueues 4 launches, every grid sized from B and the edge capacities - the live edge counts
// exist only in the sampler's meta words, so every kernel reads them there and strides:
//   mark      one WAVE per (positive, direction): the first slot of the target's row by a binary search in the list's
//             target column (the lists are sorted by target), then the 64 lanes stride over the row and overwrite the
//             source of every edge that matches with kRemoved (plain stores of one value: idempotent, so repeated
//             positives and multi-edges just mark the same slots).  The target column is never written, so searches
//             and marks of other waves on the same list do not disturb each other.
//   pack      one workgroup per chunk of 1024 slots, the types flattened into one grid: the unmarked edges of the chunk
//             go, in order, to the chunk's slots of the workspace; their number is the chunk's count.  The positives are
//             checked here as well (the status bits).
//   scan      ONE workgroup: scan of the chunk counts, the new per-type counts into meta, removed[] and the status word
//   move      chunk by chunk: the packed edges back into the list at (kept edges of earlier chunks of the type)
// Packing into the workspace first is what makes the compaction safe across workgroups: `move` reads only the workspace
// and writes only the lists.  A hub row of thousands of edges with hundreds of positives pointing at it is hundreds of
// waves striding over it.  Integers only; the only atomic is atomicOr on the status word.  Every index into a list is
// below min(live count, capacity).
#include <atomic>

#include "common.hpp"
#include "scan.hpp"

namespace tfgnn {
namespace {

constexpr int kThreads = kScanThreads;
constexpr int kWavesPerBlock = kThreads / 64;
constexpr int kMaxBlocks = 2048;
constexpr int32_t kRemoved = -2;  // a live source is a local id >= 0, or -1 where the sampler met a bad store entry

std::atomic<int64_t> g_exclude_launches;

// workspace, in int32 words: the packed edges [chunks * 1024, 2], the chunk offsets [chunks + 1]
struct Layout {
  int64_t chunks, packed, chunk_off, words;
  int32_t chunk_base[TFGNN_BATCH_MAX_EDGE_TYPES + 1];
};
// false: the capacities do not fit int32 slot offsets
inline bool layout(int L, const int64_t* edge_capacity, Layout* w) {
  int64_t chunks = 0;
  for (int t = 0; t < L; ++t) {
    w->chunk_base[t] = (int32_t)chunks;
    chunks += ceil_div(edge_capacity[t], kScanChunk);
    if (chunks * kScanChunk >= ((int64_t)1 << 31)) return false;
  }
  for (int t = L; t <= TFGNN_BATCH_MAX_EDGE_TYPES; ++t) w->chunk_base[t] = (int32_t)chunks;
  w->chunks = chunks;
  w->packed = 0;
  w->chunk_off = 2 * chunks * kScanChunk;
  w->words = w->chunk_off + (chunks + 1 + 3) / 4 * 4;
  return true;
}

struct Params {
  int L, T;
  int32_t S, B, chunks;
  const int32_t* positives;
  int32_t* meta;    // the sampler's: status, node count, [L] edge counts, hop_ptr
  int32_t* record;  // [L] removed, status
  int2* packed;
  int32_t* chunk_off;
  int32_t* adj[TFGNN_BATCH_MAX_EDGE_TYPES];
  int32_t edge_cap[TFGNN_BATCH_MAX_EDGE_TYPES];
  int32_t chunk_base[TFGNN_BATCH_MAX_EDGE_TYPES + 1];
  int8_t fwd_type[TFGNN_BATCH_MAX_EDGE_TYPES];  // processed type of relation r (-1: none); checked against L on the host
  int8_t inv_type[TFGNN_BATCH_MAX_EDGE_TYPES];
};

// the live edges of type t: the sampler's count, never beyond the capacity
__device__ __forceinline__ int32_t live_edges(const Params& P, int t) {
  return max(0, min(P.meta[TFGNN_SAMPLE_META_EDGES + t], P.edge_cap[t]));
}

// 0: row i names edges to drop; -1: the row is (-1, -1, -1), skipped in silence; otherwise the status bits of a skipped row
__device__ __forceinline__ int read_positive(const Params& P, int32_t i, int32_t* u, int32_t* r, int32_t* v) {
  const int32_t* __restrict__ row = P.positives + 3 * (int64_t)i;
  *u = row[0];
  *r = row[1];
  *v = row[2];
  if (*u == -1 && *r == -1 && *v == -1) return -1;
  int status = 0;
  if ((uint32_t)*r >= (uint32_t)P.T) status |= TFGNN_SAMPLE_EXCLUDE_BAD_RELATION;
  if ((uint32_t)*u >= (uint32_t)P.S || (uint32_t)*v >= (uint32_t)P.S) status |= TFGNN_SAMPLE_EXCLUDE_BAD_ENDPOINT;
  return status;
}

// the processed type of a flattened chunk (chunk_base is non-decreasing, chunk_base[0] = 0, fc < chunk_base[L])
__device__ __forceinline__ int type_of_chunk(const Params& P, int32_t fc) {
  int t = 0;
  while (t + 1 < P.L && fc >= P.chunk_base[t + 1]) ++t;
  return t;
}

__global__ void __launch_bounds__(kThreads) exclude_mark_kernel(const Params P) {
  if (blockIdx.x == 0 && threadIdx.x == 0) P.record[P.L] = 0;  // the status word: OR-ed into by the next launch
  const int lane = threadIdx.x & 63;
  const int64_t items = 2 * (int64_t)P.B;
  for (int64_t it = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); it < items; it += (int64_t)gridDim.x * kWavesPerBlock) {
    int32_t u, r, v;
    if (read_positive(P, (int32_t)(it >> 1), &u, &r, &v) != 0) continue;
    const bool inverse = (it & 1) != 0;
    const int t = inverse ? P.inv_type[r] : P.fwd_type[r];
    if (t < 0) continue;
    const int32_t src = inverse ? v : u, dst = inverse ? u : v;
    int32_t* __restrict__ adj = P.adj[t];
    const int32_t n = live_edges(P, t);
    int32_t lo = 0, hi = n;  // the first slot whose target is >= dst
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (adj[2 * (int64_t)mid + 1] < dst) lo = mid + 1; else hi = mid;
    }
    for (int32_t e0 = lo; e0 < n; e0 += 64) {  // the row is contiguous: stop at the first slot that is not its
      const int32_t e = e0 + lane;
      int2 edge = make_int2(-1, -1);
      const bool in_row = e < n && (edge = reinterpret_cast<const int2*>(adj)[e], edge.y == dst);
      if (in_row && edge.x == src) adj[2 * (int64_t)e] = kRemoved;
      if (!__all(in_row)) break;
    }
  }
}

__global__ void __launch_bounds__(kThreads) exclude_pack_kernel(const Params P) {
  __shared__ int32_t wave_sums[kThreads / 64];
  int status = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < P.B; i += (int64_t)gridDim.x * kThreads) {
    int32_t u, r, v;
    const int s = read_positive(P, (int32_t)i, &u, &r, &v);
    if (s > 0) status |= s;
  }
  if (status) atomicOr(P.record + P.L, status);
  for (int32_t fc = blockIdx.x; fc < P.chunks; fc += gridDim.x) {
    const int t = type_of_chunk(P, fc);
    const int32_t n = live_edges(P, t);
    const int64_t e0 = (int64_t)(fc - P.chunk_base[t]) * kScanChunk + threadIdx.x * 4;
    const int2* __restrict__ adj = reinterpret_cast<const int2*>(P.adj[t]);
    int2 edge[4];
    bool keep[4];
    int32_t kept = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      keep[q] = e0 + q < n;
      if (keep[q]) {
        edge[q] = adj[e0 + q];
        keep[q] = edge[q].x != kRemoved;
      }
      kept += keep[q];
    }
    int32_t total;
    int32_t rank = block_exclusive_scan(kept, &total, wave_sums);
    int2* __restrict__ out = P.packed + (int64_t)fc * kScanChunk;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (keep[q]) out[rank++] = edge[q];
    if (threadIdx.x == 0) P.chunk_off[fc] = total;
  }
}

__global__ void __launch_bounds__(kThreads) exclude_scan_kernel(const Params P) {
  __shared__ int32_t wave_sums[kThreads / 64];
  const int32_t total = scan_chunk_totals(P.chunk_off, P.chunks, wave_sums);
  if (threadIdx.x == 0) P.chunk_off[P.chunks] = total;
  __syncthreads();  // chunk_off is read back below by other threads of this workgroup
  const int t = threadIdx.x;
  if (t < P.L) {
    const int32_t before = live_edges(P, t);
    const int32_t now = P.chunk_off[P.chunk_base[t + 1]] - P.chunk_off[P.chunk_base[t]];
    P.record[t] = before - now;
    P.meta[TFGNN_SAMPLE_META_EDGES + t] = now;
  }
  if (t == 0) P.meta[TFGNN_SAMPLE_META_STATUS] |= P.record[P.L];  // the sampler's one copy carries the bits, too
}

__global__ void __launch_bounds__(kThreads) exclude_move_kernel(const Params P) {
  for (int32_t fc = blockIdx.x; fc < P.chunks; fc += gridDim.x) {
    const int t = type_of_chunk(P, fc);
    const int32_t kept = min(P.chunk_off[fc + 1] - P.chunk_off[fc], (int32_t)kScanChunk);
    const int32_t first = P.chunk_off[fc] - P.chunk_off[P.chunk_base[t]];  // <= the chunk's own first slot
    const int2* __restrict__ in = P.packed + (int64_t)fc * kScanChunk;
    int2* __restrict__ adj = reinterpret_cast<int2*>(P.adj[t]);
    for (int32_t i = threadIdx.x; i < kept; i += kThreads)
      if (first >= 0 && first + i < P.edge_cap[t]) adj[first + i] = in[i];
  }
}

}  // namespace
}  // namespace tfgnn

using namespace tfgnn;

extern "C" int tfgnn_sample_exclude_launch_counts(int64_t* out_counts, int n) {
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_sample_exclude_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i == 0 ? g_exclude_launches.load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

extern "C" size_t tfgnn_sample_exclude_workspace_bytes(int num_edge_types, const int64_t* edge_capacity) {
  if (num_edge_types < 0 || num_edge_types > TFGNN_BATCH_MAX_EDGE_TYPES || (num_edge_types > 0 && !edge_capacity)) return 0;
  for (int t = 0; t < num_edge_types; ++t)
    if (edge_capacity[t] < 0 || edge_capacity[t] >= ((int64_t)1 << 31)) return 0;
  Layout lay;
  if (!layout(num_edge_types, edge_capacity, &lay)) return 0;
  return (size_t)lay.words * sizeof(int32_t);
}

extern "C" int tfgnn_sample_exclude_edges(const tfgnn_sample_exclude_args* a, void* stream_) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_sample_exclude_args),
                "tfgnn_sample_exclude_edges: args is NULL or was built against another header (struct_size)");
  TFGNN_REQUIRE(a->num_edge_types >= 0 && a->num_relations >= 0 && a->num_seeds >= 0, "tfgnn_sample_exclude_edges: negative size");
  TFGNN_REQUIRE(a->num_positives >= 1, "tfgnn_sample_exclude_edges: empty batch (no positive)");
  TFGNN_REQUIRE(a->num_positives <= ((int64_t)1 << 30), "tfgnn_sample_exclude_edges: more than 2^30 positives");
  TFGNN_REQUIRE(a->num_seeds < kLimit, "tfgnn_sample_exclude_edges: 2^31 or more seeds (int32 local ids)");
  if (a->num_edge_types > TFGNN_BATCH_MAX_EDGE_TYPES || a->num_relations > TFGNN_BATCH_MAX_EDGE_TYPES) {
    set_error("tfgnn_sample_exclude_edges: at most %d edge types and relations", TFGNN_BATCH_MAX_EDGE_TYPES);
    return TFGNN_ERR_UNSUPPORTED;
  }
  const int L = a->num_edge_types, T = a->num_relations;
  TFGNN_REQUIRE(L == 0 || (a->edge_capacity && a->adjacency_lists), "tfgnn_sample_exclude_edges: NULL pointer table");
  TFGNN_REQUIRE(T == 0 || (a->fwd_type && a->inv_type), "tfgnn_sample_exclude_edges: NULL pointer table");
  for (int t = 0; t < L; ++t) {
    TFGNN_REQUIRE(a->edge_capacity[t] >= 0, "tfgnn_sample_exclude_edges: negative capacity");
    TFGNN_REQUIRE(a->edge_capacity[t] < kLimit, "tfgnn_sample_exclude_edges: an edge capacity of 2^31 or more");
  }
  for (int r = 0; r < T; ++r)
    TFGNN_REQUIRE(a->fwd_type[r] >= -1 && a->fwd_type[r] < L && a->inv_type[r] >= -1 && a->inv_type[r] < L,
                  "tfgnn_sample_exclude_edges: a type table entry must be -1 or a processed edge type in [0, %d)", L);
  TFGNN_REQUIRE(a->positives && a->meta && a->record && a->workspace, "tfgnn_sample_exclude_edges: NULL pointer");
  for (int t = 0; t < L; ++t) {
    TFGNN_REQUIRE(a->edge_capacity[t] == 0 || a->adjacency_lists[t], "tfgnn_sample_exclude_edges: NULL pointer");
    TFGNN_REQUIRE((uintptr_t)a->adjacency_lists[t] % 8 == 0, "tfgnn_sample_exclude_edges: edge lists must be 8-byte aligned");
  }
  Layout lay;
  TFGNN_REQUIRE(layout(L, a->edge_capacity, &lay), "tfgnn_sample_exclude_edges: 2^31 or more edge slots (int32 slot offsets)");
  TFGNN_REQUIRE((uintptr_t)a->workspace % 16 == 0 && a->workspace_bytes >= (size_t)lay.words * sizeof(int32_t),
                "tfgnn_sample_exclude_edges: the workspace is too small or not 16-byte aligned (tfgnn_sample_exclude_workspace_bytes)");

  Params P;
  memset(&P, 0, sizeof(P));
  P.L = L;
  P.T = T;
  P.S = (int32_t)a->num_seeds;
  P.B = (int32_t)a->num_positives;
  P.chunks = (int32_t)lay.chunks;
  P.positives = a->positives;
  P.meta = a->meta;
  P.record = a->record;
  int32_t* ws = static_cast<int32_t*>(a->workspace);
  P.packed = reinterpret_cast<int2*>(ws + lay.packed);
  P.chunk_off = ws + lay.chunk_off;
  for (int t = 0; t < L; ++t) {
    P.adj[t] = a->adjacency_lists[t];
    P.edge_cap[t] = (int32_t)a->edge_capacity[t];
  }
  for (int t = 0; t <= TFGNN_BATCH_MAX_EDGE_TYPES; ++t) P.chunk_base[t] = lay.chunk_base[t];
  for (int r = 0; r < T; ++r) {
    P.fwd_type[r] = (int8_t)a->fwd_type[r];
    P.inv_type[r] = (int8_t)a->inv_type[r];
  }

  hipStream_t stream = (hipStream_t)stream_;
  const dim3 block(kThreads);
  const unsigned chunk_grid = scan_strided_grid(lay.chunks, 1, kMaxBlocks);
  hipLaunchKernelGGL(exclude_mark_kernel, dim3(scan_strided_grid(2 * (int64_t)P.B, kWavesPerBlock, kMaxBlocks)), block, 0, stream, P);
  hipLaunchKernelGGL(exclude_pack_kernel, dim3(chunk_grid), block, 0, stream, P);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(exclude_scan_kernel, dim3(1), block, 0, stream, P);
  hipLaunchKernelGGL(exclude_move_kernel, dim3(chunk_grid), block, 0, stream, P);
  TFGNN_LAUNCH_CHECK();
  g_exclude_launches.fetch_add(TFGNN_SAMPLE_EXCLUDE_LAUNCHES, std::memory_order_relaxed);
  return TFGNN_OK;
}
