// Edge dropout (Schlichtkrull et al. 2018, section 5.2: edges dropped "before normalization"; DropEdge, Rong et al. 2020) as a
// per-step replacement of the three arrays the decomposed R-GCN layers read the graph through: tfgnn_graph_scales_edge_dropout
// draws the keep decision of every edge, recounts the kept in-degrees and writes m_v, s_e and s'_e (include/tfgnn.h has the
// contract).  Zero weights switch an edge off in basis.hip / blockdiag.hip; those kernels do not change.
//
// One launch.  One wave per target node walks the node's row of the by-target order (all in-edges, sorted by type) 64 edges
// at a time, lane i on edge i of the chunk:
//   1. mean / sqrt_n only: the kept edges of the whole row are counted first (N'_v), every lane over a 64-strided share of the
//      row, one wave sum at the end;
//   2. the chunk's keep decisions meet in one ballot; a bucket (v, l) that lies inside the chunk takes c'_{v,l} from the
//      ballot's bits.  A bucket that crosses a chunk border is counted once over its own range like the row in step 1 and
//      remembered until the walk has left it (at most two such buckets touch a chunk: the one that enters it and the one that
//      leaves it), so a hub's edges are hashed at most three times and no lane ever walks a row alone;
//   3. lane i writes s_e at its by-target position and s_e * m_v at the edge's by-source position (TFGNN_G_SRC2DST_POS's
//      inverse: part EDGE_MAPS), the only scattered access: 4 bytes per edge.
// Thresholds and kept factors of the L <= 256 types are derived once per workgroup into LDS.  Integer counts, no atomics, no
// workspace, nothing read back: the launch can be captured.
#include <atomic>

#include "common.hpp"
#include "graph.hpp"

namespace tfgnn {
namespace {

constexpr int ED_THREADS = 256;
constexpr int ED_WAVE = 64;
constexpr int ED_MAX_TYPES = 256;  // graph_create_impl refuses more

std::atomic<int64_t> g_edge_dropout_launches{0};

struct EdgeDropoutArgs {
  const int32_t* nodeptr_d;  // [V+1]
  const int32_t* rowptr_d;   // [V*L+1]
  const int32_t* coll_d;     // [E] source * L + type, by-target order
  const int32_t* eid_d;      // [E] position in concat(adjacency_lists)
  const int32_t* dst2src;    // [E] by-target position -> by-source position
  const float* rates;        // [L]
  int64_t V;
  int L, normalize, mode;
  DropoutKey key;
  float *node_scale, *ew_s, *ew_d;
};

// the header's generator section: ceil((double)rate * 2^24) of the float32 rate; outside [0, 1) clamped (NaN: 0)
__device__ __forceinline__ uint32_t edge_dropout_threshold(float rate) {
  if (!(rate > 0.f)) return 0u;
  if (rate >= 1.f) return 1u << 24;
  const double t = (double)rate * 16777216.0;
  uint32_t th = (uint32_t)t;
  if ((double)th < t) ++th;
  return th;
}

// element eid of the mask tfgnn_dropout_forward draws for this key: non-zero?
__device__ __forceinline__ bool edge_kept(const DropoutKey& k, int32_t eid, uint32_t threshold) {
  const uint32_t w = dropout_word(k, (uint64_t)((uint32_t)eid >> 2));
  return (__builtin_rotateleft32(w, 8u * ((uint32_t)eid & 3u)) >> 8) >= threshold;
}

__device__ __forceinline__ int wave_sum(int n) {
#pragma unroll
  for (int off = ED_WAVE / 2; off > 0; off >>= 1) n += __shfl_xor(n, off, ED_WAVE);
  return n;
}

// kept edges among the by-target positions [b0, b1), by the whole wave (b0, b1 and type wave-uniform; type < 0: the range
// spans buckets, every edge looks its own type up)
__device__ __forceinline__ int kept_in_range(const EdgeDropoutArgs& a, const DropoutKey& k, const uint32_t* s_threshold,
                                             int32_t b0, int32_t b1, int type, int lane) {
  int n = 0;
#pragma unroll 4
  for (int32_t q = b0 + lane; q < b1; q += ED_WAVE) {
    const int t = type >= 0 ? type : a.coll_d[q] % a.L;
    n += edge_kept(k, a.eid_d[q], s_threshold[t]) ? 1 : 0;
  }
  return wave_sum(n);
}

__global__ __launch_bounds__(ED_THREADS) void edge_dropout_scales_kernel(const EdgeDropoutArgs a) {
  __shared__ uint32_t s_threshold[ED_MAX_TYPES];
  __shared__ float s_factor[ED_MAX_TYPES];  // a kept edge's weight where no count divides
  for (int l = threadIdx.x; l < a.L; l += ED_THREADS) {
    float rate = a.rates[l];
    rate = rate > 0.f ? rate : 0.f;
    s_threshold[l] = edge_dropout_threshold(rate);
    s_factor[l] = a.mode == 0 ? 1.f / (1.f - rate) : 1.f;
  }
  __syncthreads();
  const DropoutKey k = dropout_resolve(a.key);
  const int lane = threadIdx.x % ED_WAVE;
  const int64_t waves = (int64_t)gridDim.x * (ED_THREADS / ED_WAVE);
  for (int64_t v = (int64_t)blockIdx.x * (ED_THREADS / ED_WAVE) + threadIdx.x / ED_WAVE; v < a.V; v += waves) {
    const int32_t r0 = a.nodeptr_d[v], r1 = a.nodeptr_d[v + 1];
    float m = 1.f;
    if (a.mode != 0) {  // the expressions of graph.hip's node_mult, over the kept count
      float n = (float)kept_in_range(a, k, s_threshold, r0, r1, -1, lane);
      n = n < 1.f ? 1.f : n;
      m = a.mode == 1 ? 1.f / n : 1.f / sqrtf(n);
    }
    if (lane == 0) a.node_scale[v] = m;
    int32_t span_b0 = -1;  // the border-crossing bucket counted last, and its kept count
    int span_c = 0;
    for (int32_t base = r0; base < r1; base += ED_WAVE) {
      const int32_t end = r1 - base < ED_WAVE ? r1 : base + ED_WAVE;
      const int32_t q = base + lane;
      const bool live = q < end;
      int t = 0;
      int32_t b0 = base, b1 = end;
      bool kept = false;
      if (live) {
        t = a.coll_d[q] % a.L;
        kept = edge_kept(k, a.eid_d[q], s_threshold[t]);
      }
      float s = kept ? s_factor[t] : 0.f;
      if (a.normalize) {  // wave-uniform from here to the stores
        if (live) {
          const int64_t r = v * a.L + t;
          b0 = a.rowptr_d[r];
          b1 = a.rowptr_d[r + 1];
        }
        const unsigned long long bits = __ballot(kept);
        const int lo = (b0 > base ? b0 : base) - base, hi = (b1 < end ? b1 : end) - base;  // 0 <= lo < hi <= 64
        const unsigned long long upto_hi = hi >= 64 ? ~0ull : (1ull << hi) - 1ull;
        int c = __popcll(bits & upto_hi & ~((1ull << lo) - 1ull));
        // the bucket that enters the chunk (lane 0's) and the one that leaves it (the last live lane's)
        const int last = end - base - 1;
        const int32_t in_b0 = __shfl(b0, 0, ED_WAVE), in_b1 = __shfl(b1, 0, ED_WAVE);
        const int32_t out_b0 = __shfl(b0, last, ED_WAVE), out_b1 = __shfl(b1, last, ED_WAVE);
        const int in_t = __shfl(t, 0, ED_WAVE), out_t = __shfl(t, last, ED_WAVE);
        if (in_b0 < base || in_b1 > end) {
          if (in_b0 != span_b0) {
            span_c = kept_in_range(a, k, s_threshold, in_b0, in_b1, in_t, lane);
            span_b0 = in_b0;
          }
          if (b0 == in_b0) c = span_c;
        }
        if (out_b0 != in_b0 && out_b1 > end) {
          span_c = kept_in_range(a, k, s_threshold, out_b0, out_b1, out_t, lane);
          span_b0 = out_b0;
          if (b0 == out_b0) c = span_c;
        }
        s = kept ? 1.f / ((float)c + kSmallNumber) : 0.f;
      }
      if (live) {
        a.ew_d[q] = s;
        a.ew_s[a.dst2src[q]] = s * m;
      }
    }
  }
}

}  // namespace
}  // namespace tfgnn

extern "C" int tfgnn_graph_scales_edge_dropout(const tfgnn_graph* g, int normalize_by_num_incoming, int aggregation_mode,
                                               const float* d_rates, uint64_t seed, float* d_node_scale,
                                               float* d_edge_weight_by_src, float* d_edge_weight_by_dst, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(g != nullptr, "tfgnn_graph_scales_edge_dropout: graph is NULL");
  TFGNN_REQUIRE(aggregation_mode >= 0 && aggregation_mode <= 2, "tfgnn_graph_scales_edge_dropout: unknown aggregation mode %d",
                aggregation_mode);
  TFGNN_REQUIRE((g->V == 0 || d_node_scale) && (g->E == 0 || (d_edge_weight_by_src && d_edge_weight_by_dst)),
                "tfgnn_graph_scales_edge_dropout: NULL output");
  TFGNN_REQUIRE(g->L == 0 || d_rates, "tfgnn_graph_scales_edge_dropout: d_rates is NULL");
  TFGNN_REQUIRE(g->L <= ED_MAX_TYPES, "tfgnn_graph_scales_edge_dropout: at most %d edge types", ED_MAX_TYPES);
  if (g->V == 0) return TFGNN_OK;
  if (g->E > 0) {
    const int rc = graph_require_parts(g, TFGNN_GRAPH_PART_EDGE_MAPS | TFGNN_GRAPH_PART_EDGE_IDS, "tfgnn_graph_scales_edge_dropout");
    if (rc) return rc;
  }
  EdgeDropoutArgs a;
  a.nodeptr_d = g->nodeptr_d;
  a.rowptr_d = g->rowptr_d;
  a.coll_d = g->coll_d;
  a.eid_d = g->eid_d;
  a.dst2src = g->dst2src;
  a.rates = d_rates;
  a.V = g->V;
  a.L = g->L;
  a.normalize = normalize_by_num_incoming ? 1 : 0;
  a.mode = aggregation_mode;
  a.key = dropout_key(seed, 0.f);  // the key words; every type's threshold comes from d_rates on the device
  a.key.epoch = dropout_epoch_word();
  TFGNN_REQUIRE(a.key.epoch, "tfgnn_graph_scales_edge_dropout: no device memory for the epoch word");
  a.node_scale = d_node_scale;
  a.ew_s = d_edge_weight_by_src;
  a.ew_d = d_edge_weight_by_dst;
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(g->V, ED_THREADS / ED_WAVE), 8192);
  hipLaunchKernelGGL(edge_dropout_scales_kernel, dim3(blocks), dim3(ED_THREADS), 0, (hipStream_t)stream, a);
  TFGNN_LAUNCH_CHECK();
  g_edge_dropout_launches.fetch_add(1, std::memory_order_relaxed);
  return TFGNN_OK;
}

extern "C" int tfgnn_edge_dropout_launch_counts(int64_t* out_counts, int n) {
  using namespace tfgnn;
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_edge_dropout_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i < 1 ? g_edge_dropout_launches.load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}
