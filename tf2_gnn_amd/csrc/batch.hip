// Batch assembly from a device-resident fold (include/tfgnn.h "Batch assembly from a device-resident fold").
//
// One launch per batch.  The grid is cut into parts, in this order: one run of tiles per node array (the features, then
// every node column), one run of tiles per edge type, the per-graph columns; `part_end` holds the running block counts and
// a workgroup finds its part with a scalar scan.
//   node tile      rows_per_tile batch rows of ONE node array (source, destination, width W, rows per tile, float4 flag).
//                  One thread per row finds the row's position with a binary search in the epoch's node prefix sums and
//                  leaves the row's source row in LDS - the tiles of array 0, the features, also write node_to_graph_map;
//                  then the whole workgroup copies the tile's rows_per_tile * W floats, consecutive lanes on consecutive
//                  floats of the output (and of the source within a graph).  float4 when the array's rows allow it.
//   edge tile      kEdgesPerTile edges of one type, one int2 load and one int2 store per edge, binary search in that type's
//                  prefix sums.
//   column tile    256 (graph, column) pairs.
// Every read of the store goes through an index that was checked against the store's sizes; every write is below the
// output size the host passed.
#include <atomic>

#include "common.hpp"

namespace tfgnn {

constexpr int kBatchThreads = 256;
constexpr int kEdgesPerTile = 1024;
constexpr int kFeatTileElems = 8192;  // floats one workgroup copies (32 per thread) unless a single row is longer

static std::atomic<int64_t> g_batch_launches;

struct BatchEdgeType {
  const int32_t* edge_ptr;      // store [N + 1]
  const int32_t* edges;         // store [*, 2]
  const int32_t* pos_edge_ptr;  // epoch [P + 1]
  int32_t* out;                 // [E_t, 2]
  int32_t num_edges;            // E_t
};

struct BatchNodeArray {
  const float* src;  // store [store_nodes, W]
  float* dst;        // [V, W]
  int32_t W;
  int rows_per_tile, vec4;
};

constexpr int kMaxNodeArrays = 1 + TFGNN_BATCH_MAX_NODE_COLUMNS;  // the features and the node columns

struct BatchParams {
  int num_node_arrays, num_edge_types, num_columns;
  int32_t N, store_nodes;
  int32_t p0, p1, V;
  const int32_t* node_ptr;
  const int32_t* order;
  const int32_t* pos_node_ptr;
  int32_t* node_to_graph_map;
  int* bad;
  // blocks up to and including: features, node column 0.., type 0.., columns
  uint32_t part_end[kMaxNodeArrays + TFGNN_BATCH_MAX_EDGE_TYPES + 1];
  BatchNodeArray arrays[kMaxNodeArrays];
  BatchEdgeType types[TFGNN_BATCH_MAX_EDGE_TYPES];
  const float* columns[TFGNN_BATCH_MAX_COLUMNS];
  float* column_out[TFGNN_BATCH_MAX_COLUMNS];
};

// the position p in [p0, p1) with ptr[p] <= x < ptr[p + 1]  (x in [ptr[p0], ptr[p1]); zero-length segments are skipped)
__device__ __forceinline__ int position_of(const int32_t* __restrict__ ptr, int p0, int p1, int32_t x) {
  int lo = p0, hi = p1;  // invariant: ptr[lo] <= x < ptr[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ptr[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void batch_node_tile(const BatchParams& P, const BatchNodeArray& A, bool write_map, uint32_t tile,
                                                int32_t* src_rows) {
  const int32_t base = P.pos_node_ptr[P.p0];
  const int32_t dev_V = P.pos_node_ptr[P.p1] - base;
  const int32_t r0 = (int32_t)tile * A.rows_per_tile;
  const int rows = min(A.rows_per_tile, P.V - r0);
  for (int i = threadIdx.x; i < rows; i += kBatchThreads) {
    const int32_t r = r0 + i;
    int32_t src = -1;
    if (r < dev_V) {
      const int p = position_of(P.pos_node_ptr, P.p0, P.p1, base + r);
      const int32_t g = P.order[p];
      if ((uint32_t)g < (uint32_t)P.N) {
        const int32_t s = P.node_ptr[g] + (base + r - P.pos_node_ptr[p]);
        if ((uint32_t)s < (uint32_t)P.store_nodes && s < P.node_ptr[g + 1]) {
          src = s;
          if (write_map) P.node_to_graph_map[r] = p - P.p0;
        }
      }
    }
    if (src < 0 && P.bad) *P.bad = 1;
    src_rows[i] = src;
  }
  __syncthreads();
  if (A.vec4) {
    const uint32_t F4 = (uint32_t)A.W >> 2;
    const uint32_t n = (uint32_t)rows * F4;
    const float4* __restrict__ in = reinterpret_cast<const float4*>(A.src);
    float4* __restrict__ out = reinterpret_cast<float4*>(A.dst) + (int64_t)r0 * F4;
    for (uint32_t e = threadIdx.x; e < n; e += kBatchThreads) {
      const uint32_t row = e / F4, c = e - row * F4;
      const int32_t s = src_rows[row];
      if (s >= 0) out[e] = in[(int64_t)s * F4 + c];
    }
  } else {
    const uint32_t F = (uint32_t)A.W;
    const uint32_t n = (uint32_t)rows * F;
    const float* __restrict__ in = A.src;
    float* __restrict__ out = A.dst + (int64_t)r0 * F;
    for (uint32_t e = threadIdx.x; e < n; e += kBatchThreads) {
      const uint32_t row = e / F, c = e - row * F;
      const int32_t s = src_rows[row];
      if (s >= 0) out[e] = in[(int64_t)s * F + c];
    }
  }
}

__device__ __forceinline__ void batch_edge_tile(const BatchParams& P, const BatchEdgeType& T, uint32_t tile) {
  const int32_t base = T.pos_edge_ptr[P.p0];
  const int32_t dev_E = T.pos_edge_ptr[P.p1] - base;
  const int32_t node_base = P.pos_node_ptr[P.p0];
  const int64_t e0 = (int64_t)tile * kEdgesPerTile;
  const int32_t e1 = (int32_t)min(e0 + kEdgesPerTile, (int64_t)T.num_edges);  // the sum may pass 2^31, the minimum cannot
  for (int32_t e = (int32_t)e0 + threadIdx.x; e < e1; e += kBatchThreads) {
    bool ok = false;
    if (e < dev_E) {
      const int p = position_of(T.pos_edge_ptr, P.p0, P.p1, base + e);
      const int32_t g = P.order[p];
      if ((uint32_t)g < (uint32_t)P.N) {
        const int32_t s = T.edge_ptr[g] + (base + e - T.pos_edge_ptr[p]);
        if (s >= 0 && s < T.edge_ptr[g + 1]) {
          const int2 le = reinterpret_cast<const int2*>(T.edges)[s];
          const int32_t n = P.node_ptr[g + 1] - P.node_ptr[g];
          const int32_t off = P.pos_node_ptr[p] - node_base;
          ok = (uint32_t)le.x < (uint32_t)n && (uint32_t)le.y < (uint32_t)n;
          reinterpret_cast<int2*>(T.out)[e] = make_int2(le.x + off, le.y + off);
        }
      }
    }
    if (!ok && P.bad) *P.bad = 1;
  }
}

__device__ __forceinline__ void batch_column_tile(const BatchParams& P, uint32_t tile) {
  const int32_t G = P.p1 - P.p0;
  const int64_t n = (int64_t)G * P.num_columns;
  const int64_t i = (int64_t)tile * kBatchThreads + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i / G);
  const int32_t k = (int32_t)(i - (int64_t)c * G);
  const int32_t g = P.order[P.p0 + k];
  if ((uint32_t)g < (uint32_t)P.N)
    P.column_out[c][k] = P.columns[c][g];
  else if (P.bad)
    *P.bad = 1;
}

__global__ void __launch_bounds__(kBatchThreads) batch_assemble_kernel(const BatchParams P) {
  __shared__ int32_t src_rows[kBatchThreads];
  const uint32_t b = blockIdx.x;
  const int K = P.num_node_arrays;
  for (int a = 0; a < K; ++a) {
    if (b < P.part_end[a]) {
      batch_node_tile(P, P.arrays[a], a == 0, a ? b - P.part_end[a - 1] : b, src_rows);
      return;
    }
  }
  for (int t = 0; t < P.num_edge_types; ++t) {
    if (b < P.part_end[K + t]) {
      batch_edge_tile(P, P.types[t], b - P.part_end[K + t - 1]);
      return;
    }
  }
  batch_column_tile(P, b - P.part_end[K + P.num_edge_types - 1]);
}
}  // namespace tfgnn

extern "C" int tfgnn_batch_assemble_launch_counts(int64_t* out_counts, int n) {
  using namespace tfgnn;
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_batch_assemble_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i == 0 ? g_batch_launches.load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

extern "C" int tfgnn_batch_assemble(const tfgnn_batch_assemble_args* a, void* stream) {
  using namespace tfgnn;
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_batch_assemble_args),
                "tfgnn_batch_assemble: args is NULL or was built against another header (struct_size)");
  TFGNN_REQUIRE(a->num_edge_types >= 0 && a->num_columns >= 0 && a->num_graphs >= 0 && a->store_nodes >= 0 && a->order_len >= 0 &&
                    a->num_nodes >= 0 && a->p0 >= 0 && a->p1 >= 0 && a->num_node_columns >= 0,
                "tfgnn_batch_assemble: negative size");
  TFGNN_REQUIRE(a->p0 <= a->p1, "tfgnn_batch_assemble: p0 > p1");
  TFGNN_REQUIRE(a->p1 <= a->order_len, "tfgnn_batch_assemble: p1 beyond the order");
  TFGNN_REQUIRE(a->feature_dim >= 1 && a->feature_dim < kLimit, "tfgnn_batch_assemble: feature_dim must be in [1, 2^31)");
  TFGNN_REQUIRE(a->store_nodes < kLimit && a->num_nodes < kLimit && a->num_graphs < kLimit - 1 && a->order_len < kLimit - 1,
                "tfgnn_batch_assemble: 2^31 or more nodes or graphs (int32 node ids)");
  if (a->num_edge_types > TFGNN_BATCH_MAX_EDGE_TYPES || a->num_columns > TFGNN_BATCH_MAX_COLUMNS ||
      a->num_node_columns > TFGNN_BATCH_MAX_NODE_COLUMNS) {
    set_error("tfgnn_batch_assemble: at most %d edge types, %d columns and %d node columns", TFGNN_BATCH_MAX_EDGE_TYPES,
              TFGNN_BATCH_MAX_COLUMNS, TFGNN_BATCH_MAX_NODE_COLUMNS);
    return TFGNN_ERR_UNSUPPORTED;
  }
  const int L = a->num_edge_types, C = a->num_columns, NC = a->num_node_columns;
  TFGNN_REQUIRE(L == 0 || (a->edge_ptr && a->edges && a->pos_edge_ptr && a->adjacency_lists && a->num_edges),
                "tfgnn_batch_assemble: NULL pointer table");
  TFGNN_REQUIRE(C == 0 || (a->columns && a->column_out), "tfgnn_batch_assemble: NULL pointer table");
  TFGNN_REQUIRE(NC == 0 || (a->node_column_widths && a->node_columns && a->node_column_out),
                "tfgnn_batch_assemble: NULL pointer table");
  for (int c = 0; c < NC; ++c)
    TFGNN_REQUIRE(a->node_column_widths[c] >= 1 && a->node_column_widths[c] < kLimit,
                  "tfgnn_batch_assemble: a node column width must be in [1, 2^31)");
  for (int t = 0; t < L; ++t) {
    TFGNN_REQUIRE(a->num_edges[t] >= 0, "tfgnn_batch_assemble: negative size");
    TFGNN_REQUIRE(a->num_edges[t] < kLimit, "tfgnn_batch_assemble: 2^31 or more edges of a type in one batch");
    TFGNN_REQUIRE(((uintptr_t)a->edges[t] | (uintptr_t)a->adjacency_lists[t]) % 8 == 0,
                  "tfgnn_batch_assemble: edge lists must be 8-byte aligned");
  }
  const int64_t G = a->p1 - a->p0;
  if (G == 0) {
    TFGNN_REQUIRE(a->num_nodes == 0, "tfgnn_batch_assemble: an empty batch has no nodes");
    for (int t = 0; t < L; ++t) TFGNN_REQUIRE(a->num_edges[t] == 0, "tfgnn_batch_assemble: an empty batch has no edges");
    return TFGNN_OK;
  }
  TFGNN_REQUIRE(a->order && a->pos_node_ptr && a->node_ptr, "tfgnn_batch_assemble: NULL pointer");
  TFGNN_REQUIRE(a->num_nodes == 0 || (a->features && a->node_features && a->node_to_graph_map), "tfgnn_batch_assemble: NULL pointer");
  for (int t = 0; t < L; ++t)
    TFGNN_REQUIRE(a->pos_edge_ptr[t] && a->edge_ptr[t] && (a->num_edges[t] == 0 || (a->edges[t] && a->adjacency_lists[t])),
                  "tfgnn_batch_assemble: NULL pointer");
  for (int c = 0; c < C; ++c) TFGNN_REQUIRE(a->columns[c] && a->column_out[c], "tfgnn_batch_assemble: NULL pointer");
  for (int c = 0; c < NC; ++c)
    TFGNN_REQUIRE(a->num_nodes == 0 || (a->node_columns[c] && a->node_column_out[c]), "tfgnn_batch_assemble: NULL pointer");

  BatchParams P;
  memset(&P, 0, sizeof(P));
  const int K = 1 + NC;
  P.num_node_arrays = K;
  P.num_edge_types = L;
  P.num_columns = C;
  P.N = (int32_t)a->num_graphs;
  P.store_nodes = (int32_t)a->store_nodes;
  P.p0 = (int32_t)a->p0;
  P.p1 = (int32_t)a->p1;
  P.V = (int32_t)a->num_nodes;
  P.node_ptr = a->node_ptr;
  P.order = a->order;
  P.pos_node_ptr = a->pos_node_ptr;
  P.node_to_graph_map = a->node_to_graph_map;
  P.bad = a->bad_flag;
  int64_t blocks = 0;
  for (int k = 0; k < K; ++k) {  // array 0: the features; 1..: the node columns
    BatchNodeArray& A = P.arrays[k];
    const int64_t W = k ? a->node_column_widths[k - 1] : a->feature_dim;
    A.src = k ? a->node_columns[k - 1] : a->features;
    A.dst = k ? a->node_column_out[k - 1] : a->node_features;
    A.W = (int32_t)W;
    A.rows_per_tile = (int)std::max<int64_t>(1, std::min<int64_t>(kBatchThreads, kFeatTileElems / W));
    A.vec4 = W % 4 == 0 && ((uintptr_t)A.src | (uintptr_t)A.dst) % 16 == 0;
    blocks += ceil_div(a->num_nodes, A.rows_per_tile);
    P.part_end[k] = (uint32_t)blocks;
  }
  for (int t = 0; t < L; ++t) {
    P.types[t].edge_ptr = a->edge_ptr[t];
    P.types[t].edges = a->edges[t];
    P.types[t].pos_edge_ptr = a->pos_edge_ptr[t];
    P.types[t].out = a->adjacency_lists[t];
    P.types[t].num_edges = (int32_t)a->num_edges[t];
    blocks += ceil_div(a->num_edges[t], kEdgesPerTile);
    P.part_end[K + t] = (uint32_t)blocks;
  }
  for (int c = 0; c < C; ++c) {
    P.columns[c] = a->columns[c];
    P.column_out[c] = a->column_out[c];
  }
  blocks += ceil_div(G * C, kBatchThreads);
  P.part_end[K + L] = (uint32_t)blocks;
  TFGNN_REQUIRE(blocks < kLimit, "tfgnn_batch_assemble: batch too large for one grid");
  if (blocks == 0) return TFGNN_OK;
  hipLaunchKernelGGL(batch_assemble_kernel, dim3((unsigned)blocks), dim3(kBatchThreads), 0, (hipStream_t)stream, P);
  TFGNN_LAUNCH_CHECK();
  g_batch_launches.fetch_add(1, std::memory_order_relaxed);
  return TFGNN_OK;
}
