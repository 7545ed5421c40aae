// K-hop neighbour sampling on a device-resident in-CSR and the row gather of a sampled batch
// (include/tfgnn.h "Neighbour sampling").
//
// tfgnn_neighbor_sample enqueues 1 + 6 K + 2 launches, every grid sized from the caller's capacities - the sizes
// themselves (frontier, edge slots, new nodes) exist only on the device, so every kernel reads them there and strides:
//   seeds            nodes[0:S] = seeds, local-id table[seed] = position, the meta words zeroed
//   per hop h:
//     count          one thread per (type, frontier node) row: c = min(d, f); exclusive scan inside chunks of 1024 rows
//     count_scan     ONE workgroup: scan of the chunk totals, the per-type starts, the new edge counts, overflow bits
//     slots          one thread per OUTPUT EDGE SLOT: row by a two-level binary search in the scanned counts, position
//                    by the keyed Feistel walk, one index load, one int2 store, and table[src] = kMarked where it was -1
//                    (plain stores of one value: idempotent)
//     mark_count     scan over the table: marked entries per chunk of 1024 ids
//     mark_scan      ONE workgroup: scan of those counts, the new node count, hop_ptr[h + 1]
//     mark_assign    scan over the table again: a marked id takes local id (nodes so far) + (its rank among the marked) -
//                    increasing global id - and goes to `nodes`; ids beyond the capacity go back to -1
//   translate        the source column of every edge: global id -> local id through the table
//   restore          table[nodes[i]] = -1
// A hub row of thousands of in-edges is thousands of independent slots, not one long loop of one wave.  No float
// arithmetic; the only atomics are atomicOr on the status word (bits: the result does not depend on their order).
// Every read of the store goes through an index checked against the store's sizes; every write is below a capacity.
#include <atomic>

#include "common.hpp"
#include "scan.hpp"

namespace tfgnn {

constexpr int kSampleThreads = kScanThreads;
constexpr int kSampleChunk = kScanChunk;  // rows (or ids) whose counts one workgroup scans: 4 per thread (csrc/scan.hpp)
constexpr int kSampleMaxBlocks = 2048;
constexpr int32_t kMarked = -2;
constexpr int kGatherTileElems = 8192;  // as kFeatTileElems of csrc/batch.hip

static std::atomic<int64_t> g_sample_launches, g_gather_rows_launches;

// workspace, in int32 words: the table [V rounded up to 4], the chunk-local scans [L * node_capacity], the row chunk
// offsets [chunks + 1], the id chunk offsets [ceil(V / 1024) + 1], the state words
struct SampleLayout {
  int64_t table, scan, chunk_off, vchunk_off, state, words;
};
constexpr int kStateTotal = 0, kStateNodesBefore = 1, kStateTypeStart = 2;  // [L + 1] type starts, then [L] edge bases
static inline int64_t state_words(int L) { return 2 + (L + 1) + L; }
static inline SampleLayout sample_layout(int64_t V, int L, int64_t node_capacity) {
  SampleLayout w;
  auto up4 = [](int64_t n) { return (n + 3) / 4 * 4; };
  w.table = 0;
  w.scan = up4(V);
  w.chunk_off = w.scan + up4(L * node_capacity);
  w.vchunk_off = w.chunk_off + up4(ceil_div(L * node_capacity, kSampleChunk) + 1);
  w.state = w.vchunk_off + up4(ceil_div(V, kSampleChunk) + 1);
  w.words = w.state + up4(state_words(L));
  return w;
}

struct SampleParams {
  int L, K;
  int32_t V, S, node_cap;
  uint32_t s0, s1;
  const int32_t* seeds;
  int32_t* nodes;
  int32_t* meta;  // status, node count, [L] edge counts, [K + 2] hop_ptr
  int32_t* table;
  int32_t* scan;
  int32_t* chunk_off;
  int32_t* vchunk_off;
  int32_t* state;
  const int32_t* in_ptr[TFGNN_BATCH_MAX_EDGE_TYPES];
  const int32_t* in_src[TFGNN_BATCH_MAX_EDGE_TYPES];
  int32_t* adj[TFGNN_BATCH_MAX_EDGE_TYPES];
  int32_t store_edges[TFGNN_BATCH_MAX_EDGE_TYPES];
  int32_t edge_cap[TFGNN_BATCH_MAX_EDGE_TYPES];
};

__device__ __forceinline__ int32_t* meta_edges(const SampleParams& P) { return P.meta + TFGNN_SAMPLE_META_EDGES; }
__device__ __forceinline__ int32_t* meta_hop_ptr(const SampleParams& P) { return P.meta + TFGNN_SAMPLE_META_EDGES + P.L; }

// in-degree of type t of node v, 0 for anything the store's sizes do not admit
__device__ __forceinline__ int32_t in_degree(const SampleParams& P, int t, int32_t v, int32_t* first) {
  const int32_t a = P.in_ptr[t][v], b = P.in_ptr[t][v + 1];
  *first = a;
  return (a >= 0 && b >= a && b <= P.store_edges[t]) ? b - a : 0;
}
__device__ __forceinline__ int32_t taken(int32_t d, int32_t f) { return (f < 0 || d <= f) ? d : f; }

// position j of a row of in-degree d under the row key k: (pi(j) + off) mod d, pi an 8-round balanced Feistel network
// on the smallest even number of bits that holds d - 1 (at least 2), cycle-walked into [0, d)
__device__ __forceinline__ uint32_t sample_position(uint32_t k, uint32_t d, uint32_t j) {
  const int bits = 32 - __builtin_clz((d - 1) | 1u);  // bit_length(d - 1), 1 for d <= 2
  const int half = max(1, (bits + 1) >> 1);
  const uint32_t mask = (1u << half) - 1u;
  uint32_t x = j;
  do {
    uint32_t l = x >> half, r = x & mask;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
      const uint32_t f = (lowbias32(r ^ (k + i * 0x9E3779B9u)) >> 7) & mask;
      const uint32_t nr = l ^ f;
      l = r;
      r = nr;
    }
    x = (l << half) | r;
  } while (x >= d);
  const uint32_t off = lowbias32(k ^ 0xA5A5A5A5u) % d;
  const uint32_t p = x + off;  // < 2 d <= 2^32 - 2
  return p >= d ? p - d : p;
}
__device__ __forceinline__ uint32_t row_key(const SampleParams& P, int32_t v, int t) {
  return lowbias32(lowbias32((uint32_t)v ^ P.s0) + (uint32_t)(t + 1) * 0x9E3779B9u) ^ P.s1;
}

__global__ void __launch_bounds__(kSampleThreads) sample_seeds_kernel(const SampleParams P) {
  const int64_t tid = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
  if (tid == 0) {
    P.meta[TFGNN_SAMPLE_META_STATUS] = 0;
    P.meta[TFGNN_SAMPLE_META_NODES] = P.S;
    int32_t* hop_ptr = meta_hop_ptr(P);
    hop_ptr[0] = 0;
    for (int h = 1; h <= P.K + 1; ++h) hop_ptr[h] = P.S;
  }
  if (tid < P.L) meta_edges(P)[tid] = 0;
  for (int64_t i = tid; i < P.S; i += (int64_t)gridDim.x * kSampleThreads) {
    const int32_t v = P.seeds[i];
    P.nodes[i] = v;
    if ((uint32_t)v < (uint32_t)P.V) P.table[v] = (int32_t)i;  // a repeated seed: one of its positions stays, hop 1 sees it
  }
}

// rows r = t * Fr + i of the frontier [f0, f0 + Fr): counts, scanned inside each chunk of 1024 rows
__global__ void __launch_bounds__(kSampleThreads) sample_count_kernel(const SampleParams P, int hop, int32_t fanout) {
  __shared__ int32_t wave_sums[kSampleThreads / 64];
  const int32_t* hop_ptr = meta_hop_ptr(P);
  const int32_t f0 = hop_ptr[hop - 1];
  const int32_t Fr = hop_ptr[hop] - f0;
  const int64_t R = (int64_t)P.L * Fr;
  const int64_t chunks = (R + kSampleChunk - 1) / kSampleChunk;
  int status = 0;
  for (int64_t ck = blockIdx.x; ck < chunks; ck += gridDim.x) {
    const int64_t r0 = ck * kSampleChunk + threadIdx.x * 4;
    int32_t c[4];
    int32_t sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t r = r0 + q;
      c[q] = 0;
      if (r < R) {
        const int t = (int)(r / Fr);
        const int32_t i = (int32_t)(r - (int64_t)t * Fr);
        const int32_t v = P.nodes[f0 + i];
        if ((uint32_t)v >= (uint32_t)P.V) {
          status |= TFGNN_SAMPLE_BAD_SEED;
        } else {
          if (hop == 1 && P.table[v] != f0 + i) status |= TFGNN_SAMPLE_REPEATED_SEED;
          int32_t first;
          c[q] = taken(in_degree(P, t, v, &first), fanout);
        }
      }
      sum += c[q];
    }
    int32_t total;
    int32_t run = block_exclusive_scan(sum, &total, wave_sums);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (r0 + q < R) P.scan[r0 + q] = run;
      run += c[q];
    }
    if (threadIdx.x == 0) P.chunk_off[ck] = total;
  }
  if (status) atomicOr(P.meta + TFGNN_SAMPLE_META_STATUS, status);
}

// one workgroup: chunk totals -> exclusive offsets (carry across rounds of 256 chunks), then the per-type bookkeeping
__global__ void __launch_bounds__(kSampleThreads) sample_count_scan_kernel(const SampleParams P, int hop) {
  __shared__ int32_t wave_sums[kSampleThreads / 64];
  const int32_t* hop_ptr = meta_hop_ptr(P);
  const int32_t Fr = hop_ptr[hop] - hop_ptr[hop - 1];
  const int64_t R = (int64_t)P.L * Fr;
  const int64_t chunks = (R + kSampleChunk - 1) / kSampleChunk;
  const int32_t carry = scan_chunk_totals(P.chunk_off, chunks, wave_sums);
  if (threadIdx.x == 0) {
    P.chunk_off[chunks] = carry;
    P.state[kStateTotal] = carry;
    P.state[kStateTypeStart + P.L] = carry;
  }
  __syncthreads();  // chunk_off is read back below by other threads of this workgroup
  const int t = threadIdx.x;
  if (t < P.L) {
    const int64_t r = (int64_t)t * Fr;
    P.state[kStateTypeStart + t] = Fr > 0 ? P.chunk_off[r / kSampleChunk] + P.scan[r] : 0;
  }
  __syncthreads();
  if (t < P.L) {
    const int32_t n = P.state[kStateTypeStart + t + 1] - P.state[kStateTypeStart + t];
    const int32_t base = meta_edges(P)[t];
    P.state[kStateTypeStart + P.L + 1 + t] = base;
    const int64_t want = (int64_t)base + n;
    if (want > P.edge_cap[t]) atomicOr(P.meta + TFGNN_SAMPLE_META_STATUS, TFGNN_SAMPLE_EDGE_OVERFLOW);
    meta_edges(P)[t] = (int32_t)min(want, (int64_t)P.edge_cap[t]);
  }
}

// the largest index i in [0, n) with a[i] <= x  (a non-decreasing, a[0] <= x)
__device__ __forceinline__ int64_t last_not_above(const int32_t* __restrict__ a, int64_t n, int32_t x) {
  int64_t lo = 0, hi = n;  // invariant: a[lo] <= x, a[hi] > x or hi == n
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kSampleThreads) sample_slots_kernel(const SampleParams P, int hop, int32_t fanout) {
  const int32_t* hop_ptr = meta_hop_ptr(P);
  const int32_t f0 = hop_ptr[hop - 1];
  const int32_t Fr = hop_ptr[hop] - f0;
  const int64_t R = (int64_t)P.L * Fr;
  const int64_t chunks = (R + kSampleChunk - 1) / kSampleChunk;
  const int32_t total = P.state[kStateTotal];
  int status = 0;
  for (int64_t e = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kSampleThreads) {
    const int64_t ck = last_not_above(P.chunk_off, chunks, (int32_t)e);
    const int32_t in_chunk = (int32_t)e - P.chunk_off[ck];
    const int64_t rows = min((int64_t)kSampleChunk, R - ck * kSampleChunk);
    const int64_t r = ck * kSampleChunk + last_not_above(P.scan + ck * kSampleChunk, rows, in_chunk);
    const int32_t row_start = P.chunk_off[ck] + P.scan[r];
    const int32_t j = (int32_t)e - row_start;
    const int t = (int)(r / Fr);
    const int32_t i = (int32_t)(r - (int64_t)t * Fr);
    const int32_t v = P.nodes[f0 + i];
    if ((uint32_t)v >= (uint32_t)P.V) continue;  // such a row counted no edges
    int32_t first;
    const int32_t d = in_degree(P, t, v, &first);
    const int32_t c = taken(d, fanout);
    if (j < 0 || j >= c) {  // the scan and the store disagree: nothing is read or written
      status |= TFGNN_SAMPLE_BAD_STORE;
      continue;
    }
    const int32_t p = c == d ? j : (int32_t)sample_position(row_key(P, v, t), (uint32_t)d, (uint32_t)j);
    const int32_t src = P.in_src[t][first + p];
    const int64_t pos = (int64_t)P.state[kStateTypeStart + P.L + 1 + t] + (row_start - P.state[kStateTypeStart + t]) + j;
    if (pos >= P.edge_cap[t]) continue;  // the overflow bit is set by the scan
    if ((uint32_t)src >= (uint32_t)P.V) {
      status |= TFGNN_SAMPLE_BAD_STORE;
      reinterpret_cast<int2*>(P.adj[t])[pos] = make_int2(-1, f0 + i);
      continue;
    }
    reinterpret_cast<int2*>(P.adj[t])[pos] = make_int2(src, f0 + i);  // the source stays global until the translate pass
    if (P.table[src] == -1) P.table[src] = kMarked;
  }
  if (status) atomicOr(P.meta + TFGNN_SAMPLE_META_STATUS, status);
}

__global__ void __launch_bounds__(kSampleThreads) sample_mark_count_kernel(const SampleParams P) {
  __shared__ int32_t wave_sums[kSampleThreads / 64];
  count_marked_chunks(P.table, P.V, kMarked, P.vchunk_off, wave_sums);
}

__global__ void __launch_bounds__(kSampleThreads) sample_mark_scan_kernel(const SampleParams P, int hop) {
  __shared__ int32_t wave_sums[kSampleThreads / 64];
  const int64_t chunks = ((int64_t)P.V + kSampleChunk - 1) / kSampleChunk;
  const int32_t carry = scan_chunk_totals(P.vchunk_off, chunks, wave_sums);
  if (threadIdx.x == 0) {
    const int32_t before = P.meta[TFGNN_SAMPLE_META_NODES];
    const int64_t want = (int64_t)before + carry;
    if (want > P.node_cap) atomicOr(P.meta + TFGNN_SAMPLE_META_STATUS, TFGNN_SAMPLE_NODE_OVERFLOW);
    const int32_t now = (int32_t)min(want, (int64_t)P.node_cap);
    P.state[kStateNodesBefore] = before;
    P.meta[TFGNN_SAMPLE_META_NODES] = now;
    int32_t* hop_ptr = meta_hop_ptr(P);
    for (int h = hop + 1; h <= P.K + 1; ++h) hop_ptr[h] = now;
  }
}

__global__ void __launch_bounds__(kSampleThreads) sample_mark_assign_kernel(const SampleParams P) {
  __shared__ int32_t wave_sums[kSampleThreads / 64];
  // a marked id takes local id (nodes so far) + (its rank among the marked); no room: back to -1
  assign_marked_chunks(P.table, P.V, kMarked, P.vchunk_off, P.state[kStateNodesBefore], P.node_cap, P.nodes, wave_sums);
}

__global__ void __launch_bounds__(kSampleThreads) sample_translate_kernel(const SampleParams P) {
  for (int t = 0; t < P.L; ++t) {
    const int32_t n = meta_edges(P)[t];
    int32_t* __restrict__ adj = P.adj[t];
    for (int64_t e = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kSampleThreads) {
      const int32_t src = adj[2 * e];
      adj[2 * e] = (uint32_t)src < (uint32_t)P.V ? P.table[src] : -1;
    }
  }
}

__global__ void __launch_bounds__(kSampleThreads) sample_restore_kernel(const SampleParams P) {
  const int32_t n = P.meta[TFGNN_SAMPLE_META_NODES];
  for (int64_t i = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSampleThreads) {
    const int32_t v = P.nodes[i];
    if ((uint32_t)v < (uint32_t)P.V) P.table[v] = -1;
  }
}

// ---- row gather -------------------------------------------------------------------------------------------------------------
struct GatherArray {
  const float* src;  // store [store_nodes, W]
  float* dst;        // [n, W]
  int32_t W;
  int rows_per_tile, vec4, seed_only;
};
struct GatherParams {
  int num_arrays;
  int32_t store_nodes, n, S;
  const int32_t* nodes;
  int* bad;
  uint32_t part_end[1 + TFGNN_BATCH_MAX_NODE_COLUMNS];
  GatherArray arrays[1 + TFGNN_BATCH_MAX_NODE_COLUMNS];
};

constexpr int32_t kRowZero = -1, kRowSkip = -2;

__global__ void __launch_bounds__(kSampleThreads) gather_node_rows_kernel(const GatherParams P) {
  __shared__ int32_t src_rows[kSampleThreads];
  const uint32_t b = blockIdx.x;
  int a = 0;
  while (a + 1 < P.num_arrays && b >= P.part_end[a]) ++a;
  const GatherArray& A = P.arrays[a];
  const uint32_t tile = a ? b - P.part_end[a - 1] : b;
  const int32_t r0 = (int32_t)tile * A.rows_per_tile;
  const int rows = min(A.rows_per_tile, P.n - r0);
  for (int i = threadIdx.x; i < rows; i += kSampleThreads) {
    const int32_t r = r0 + i;
    int32_t src = kRowZero;
    if (!(A.seed_only && r >= P.S)) {
      src = P.nodes[r];
      if ((uint32_t)src >= (uint32_t)P.store_nodes) {
        src = kRowSkip;
        if (P.bad) *P.bad = 1;
      }
    }
    src_rows[i] = src;
  }
  __syncthreads();
  if (A.vec4) {
    const uint32_t F4 = (uint32_t)A.W >> 2;
    const uint32_t n = (uint32_t)rows * F4;
    const float4* __restrict__ in = reinterpret_cast<const float4*>(A.src);
    float4* __restrict__ out = reinterpret_cast<float4*>(A.dst) + (int64_t)r0 * F4;
    for (uint32_t e = threadIdx.x; e < n; e += kSampleThreads) {
      const uint32_t row = e / F4, c = e - row * F4;
      const int32_t s = src_rows[row];
      if (s >= 0) out[e] = in[(int64_t)s * F4 + c];
      else if (s == kRowZero) out[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  } else {
    const uint32_t F = (uint32_t)A.W;
    const uint32_t n = (uint32_t)rows * F;
    const float* __restrict__ in = A.src;
    float* __restrict__ out = A.dst + (int64_t)r0 * F;
    for (uint32_t e = threadIdx.x; e < n; e += kSampleThreads) {
      const uint32_t row = e / F, c = e - row * F;
      const int32_t s = src_rows[row];
      if (s >= 0) out[e] = in[(int64_t)s * F + c];
      else if (s == kRowZero) out[e] = 0.f;
    }
  }
}

static inline unsigned strided_grid(int64_t items, int64_t per_block) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, per_block), kSampleMaxBlocks));
}
}  // namespace tfgnn

extern "C" int tfgnn_sample_launch_counts(int64_t* out_counts, int n) {
  using namespace tfgnn;
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_sample_launch_counts: bad argument");
  for (int i = 0; i < n; ++i)
    out_counts[i] = i == 0 ? g_sample_launches.load(std::memory_order_relaxed)
                           : i == 1 ? g_gather_rows_launches.load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

extern "C" size_t tfgnn_neighbor_sample_workspace_bytes(int64_t num_nodes, int num_edge_types, int64_t node_capacity) {
  using namespace tfgnn;
  if (num_nodes < 0 || num_nodes >= ((int64_t)1 << 31) || num_edge_types < 0 || num_edge_types > TFGNN_BATCH_MAX_EDGE_TYPES ||
      node_capacity < 0 || node_capacity > num_nodes)
    return 0;
  return (size_t)sample_layout(num_nodes, num_edge_types, node_capacity).words * sizeof(int32_t);
}

extern "C" int tfgnn_neighbor_sample(const tfgnn_neighbor_sample_args* a, void* stream_) {
  using namespace tfgnn;
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_neighbor_sample_args),
                "tfgnn_neighbor_sample: args is NULL or was built against another header (struct_size)");
  TFGNN_REQUIRE(a->num_hops >= 1 && a->num_hops <= TFGNN_SAMPLE_MAX_HOPS, "tfgnn_neighbor_sample: num_hops must be in [1, %d]",
                TFGNN_SAMPLE_MAX_HOPS);
  TFGNN_REQUIRE(a->num_seeds >= 1, "tfgnn_neighbor_sample: at least one seed");
  TFGNN_REQUIRE(a->num_nodes >= 1 && a->num_edge_types >= 0, "tfgnn_neighbor_sample: negative size");
  TFGNN_REQUIRE(a->num_nodes < kLimit, "tfgnn_neighbor_sample: 2^31 or more nodes (int32 node ids)");
  if (a->num_edge_types > TFGNN_BATCH_MAX_EDGE_TYPES) {
    set_error("tfgnn_neighbor_sample: at most %d edge types", TFGNN_BATCH_MAX_EDGE_TYPES);
    return TFGNN_ERR_UNSUPPORTED;
  }
  const int L = a->num_edge_types, K = a->num_hops;
  TFGNN_REQUIRE(a->node_capacity >= 0, "tfgnn_neighbor_sample: negative capacity");
  TFGNN_REQUIRE(L == 0 || (a->in_ptr && a->in_src && a->store_edges && a->edge_capacity && a->adjacency_lists),
                "tfgnn_neighbor_sample: NULL pointer table");
  int64_t store_total = 0;
  for (int t = 0; t < L; ++t) {
    TFGNN_REQUIRE(a->edge_capacity[t] >= 0, "tfgnn_neighbor_sample: negative capacity");
    TFGNN_REQUIRE(a->store_edges[t] >= 0, "tfgnn_neighbor_sample: negative size");
    store_total += a->store_edges[t];
    TFGNN_REQUIRE(store_total < kLimit, "tfgnn_neighbor_sample: 2^31 or more edges in the store (int32 slot offsets)");
    TFGNN_REQUIRE(a->edge_capacity[t] < kLimit, "tfgnn_neighbor_sample: an edge capacity of 2^31 or more");
  }
  TFGNN_REQUIRE(a->num_seeds <= a->node_capacity && a->node_capacity <= a->num_nodes,
                "tfgnn_neighbor_sample: the node capacity must hold the seeds and is at most the number of nodes");
  TFGNN_REQUIRE(a->fanouts && a->seeds && a->nodes && a->meta && a->workspace, "tfgnn_neighbor_sample: NULL pointer");
  for (int t = 0; t < L; ++t) {
    TFGNN_REQUIRE(a->in_ptr[t] && (a->store_edges[t] == 0 || a->in_src[t]) && (a->edge_capacity[t] == 0 || a->adjacency_lists[t]),
                  "tfgnn_neighbor_sample: NULL pointer");
    TFGNN_REQUIRE((uintptr_t)a->adjacency_lists[t] % 8 == 0, "tfgnn_neighbor_sample: edge lists must be 8-byte aligned");
  }
  const SampleLayout lay = sample_layout(a->num_nodes, L, a->node_capacity);
  TFGNN_REQUIRE((uintptr_t)a->workspace % 16 == 0 && a->workspace_bytes >= (size_t)lay.words * sizeof(int32_t),
                "tfgnn_neighbor_sample: the workspace is too small or not 16-byte aligned (tfgnn_neighbor_sample_workspace_bytes)");

  SampleParams P;
  memset(&P, 0, sizeof(P));
  P.L = L;
  P.K = K;
  P.V = (int32_t)a->num_nodes;
  P.S = (int32_t)a->num_seeds;
  P.node_cap = (int32_t)a->node_capacity;
  const DropoutKey key = dropout_key(a->seed, 0.f);  // the splitmix64 step; rate 0 touches no device memory
  P.s0 = key.s0;
  P.s1 = key.s1;
  P.seeds = a->seeds;
  P.nodes = a->nodes;
  P.meta = a->meta;
  int32_t* ws = static_cast<int32_t*>(a->workspace);
  P.table = ws + lay.table;
  P.scan = ws + lay.scan;
  P.chunk_off = ws + lay.chunk_off;
  P.vchunk_off = ws + lay.vchunk_off;
  P.state = ws + lay.state;
  int64_t edge_cap_total = 0;
  for (int t = 0; t < L; ++t) {
    P.in_ptr[t] = a->in_ptr[t];
    P.in_src[t] = a->in_src[t];
    P.adj[t] = a->adjacency_lists[t];
    P.store_edges[t] = (int32_t)a->store_edges[t];
    P.edge_cap[t] = (int32_t)a->edge_capacity[t];
    edge_cap_total += std::min(a->edge_capacity[t], a->store_edges[t]);
  }
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 block(kSampleThreads);
  const unsigned row_grid = strided_grid((int64_t)L * P.node_cap, kSampleChunk);
  const unsigned slot_grid = strided_grid(edge_cap_total, kSampleThreads);
  const unsigned id_grid = strided_grid(P.V, kSampleChunk);
  hipLaunchKernelGGL(sample_seeds_kernel, dim3(strided_grid(std::max<int64_t>(P.S, L), kSampleThreads)), block, 0, stream, P);
  TFGNN_LAUNCH_CHECK();
  for (int h = 1; h <= K; ++h) {
    const int32_t f = a->fanouts[h - 1];
    hipLaunchKernelGGL(sample_count_kernel, dim3(row_grid), block, 0, stream, P, h, f);
    hipLaunchKernelGGL(sample_count_scan_kernel, dim3(1), block, 0, stream, P, h);
    hipLaunchKernelGGL(sample_slots_kernel, dim3(slot_grid), block, 0, stream, P, h, f);
    hipLaunchKernelGGL(sample_mark_count_kernel, dim3(id_grid), block, 0, stream, P);
    hipLaunchKernelGGL(sample_mark_scan_kernel, dim3(1), block, 0, stream, P, h);
    hipLaunchKernelGGL(sample_mark_assign_kernel, dim3(id_grid), block, 0, stream, P);
    TFGNN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sample_translate_kernel, dim3(slot_grid), block, 0, stream, P);
  hipLaunchKernelGGL(sample_restore_kernel, dim3(strided_grid(P.node_cap, kSampleThreads)), block, 0, stream, P);
  TFGNN_LAUNCH_CHECK();
  g_sample_launches.fetch_add(3 + 6 * K, std::memory_order_relaxed);
  return TFGNN_OK;
}

extern "C" int tfgnn_gather_node_rows(const tfgnn_gather_node_rows_args* a, void* stream) {
  using namespace tfgnn;
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_gather_node_rows_args),
                "tfgnn_gather_node_rows: args is NULL or was built against another header (struct_size)");
  TFGNN_REQUIRE(a->store_nodes >= 0 && a->num_rows >= 0 && a->num_seeds >= 0 && a->num_node_columns >= 0,
                "tfgnn_gather_node_rows: negative size");
  TFGNN_REQUIRE(a->store_nodes < kLimit && a->num_rows < kLimit, "tfgnn_gather_node_rows: 2^31 or more nodes (int32 node ids)");
  TFGNN_REQUIRE(a->feature_dim >= 1 && a->feature_dim < kLimit, "tfgnn_gather_node_rows: feature_dim must be in [1, 2^31)");
  if (a->num_node_columns > TFGNN_BATCH_MAX_NODE_COLUMNS) {
    set_error("tfgnn_gather_node_rows: at most %d node columns", TFGNN_BATCH_MAX_NODE_COLUMNS);
    return TFGNN_ERR_UNSUPPORTED;
  }
  const int NC = a->num_node_columns;
  TFGNN_REQUIRE(NC == 0 || (a->node_column_widths && a->node_columns && a->node_column_out && a->seed_only),
                "tfgnn_gather_node_rows: NULL pointer table");
  for (int c = 0; c < NC; ++c)
    TFGNN_REQUIRE(a->node_column_widths[c] >= 1 && a->node_column_widths[c] < kLimit,
                  "tfgnn_gather_node_rows: a node column width must be in [1, 2^31)");
  if (a->num_rows == 0) return TFGNN_OK;
  TFGNN_REQUIRE(a->nodes && a->features && a->node_features, "tfgnn_gather_node_rows: NULL pointer");
  for (int c = 0; c < NC; ++c) TFGNN_REQUIRE(a->node_columns[c] && a->node_column_out[c], "tfgnn_gather_node_rows: NULL pointer");

  GatherParams P;
  memset(&P, 0, sizeof(P));
  P.num_arrays = 1 + NC;
  P.store_nodes = (int32_t)a->store_nodes;
  P.n = (int32_t)a->num_rows;
  P.S = (int32_t)std::min(a->num_seeds, a->num_rows);
  P.nodes = a->nodes;
  P.bad = a->bad_flag;
  int64_t blocks = 0;
  for (int k = 0; k <= NC; ++k) {  // array 0: the features; 1..: the node columns
    GatherArray& A = P.arrays[k];
    const int64_t W = k ? a->node_column_widths[k - 1] : a->feature_dim;
    A.src = k ? a->node_columns[k - 1] : a->features;
    A.dst = k ? a->node_column_out[k - 1] : a->node_features;
    A.W = (int32_t)W;
    A.rows_per_tile = (int)std::max<int64_t>(1, std::min<int64_t>(kSampleThreads, kGatherTileElems / W));
    A.vec4 = W % 4 == 0 && ((uintptr_t)A.src | (uintptr_t)A.dst) % 16 == 0;
    A.seed_only = k ? a->seed_only[k - 1] != 0 : 0;
    blocks += ceil_div(a->num_rows, A.rows_per_tile);
    P.part_end[k] = (uint32_t)blocks;
  }
  TFGNN_REQUIRE(blocks < kLimit, "tfgnn_gather_node_rows: too many rows for one grid");
  hipLaunchKernelGGL(gather_node_rows_kernel, dim3((unsigned)blocks), dim3(kSampleThreads), 0, (hipStream_t)stream, P);
  TFGNN_LAUNCH_CHECK();
  g_gather_rows_launches.fetch_add(1, std::memory_order_relaxed);
  return TFGNN_OK;
}
