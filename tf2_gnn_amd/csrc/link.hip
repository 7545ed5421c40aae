// Link prediction with a DistMult decoder (LinkPredictionTask; the reference has no counterpart, PARITY UNPINNED): the score
// of a typed edge (u, t, v) from the final node representations, s = sum_d H[u, d] R[t, d] H[v, d].
//   tfgnn_distmult_ce_metrics: scores, weighted sigmoid cross-entropy, confusion counts, d loss / d score
//   tfgnn_distmult_backward:   d loss / d H (a CSR row walk over the triples of every node) and d loss / d R (over the triples
//                              of every relation)
//   tfgnn_distmult_rank:       for evaluation, how many candidate entities score above / equal to the true one
// The contracts are the comments in include/tfgnn.h.  Every score of every kernel comes out of distmult_score below; no
// floating-point atomic anywhere: every sum has an order fixed by the arguments and the tables.  The ranking counts are exact
// integers (integer atomics).  All passes are bandwidth / latency bound row walks; no product kernel is involved.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "common.hpp"

namespace tfgnn {
namespace {

constexpr int LINK_BLOCKS = 1024;        // partials of the forward main pass
constexpr int LINK_WEIGHT_BLOCKS = 64;   // partials of the weight pre-pass: one per lane of the wave that adds them up
constexpr int LINK_CHUNK = 256;          // entries (triples) per chunk of the backward passes
constexpr int LINK_HALF = LINK_CHUNK / 2;
constexpr int LINK_COLS = 256;           // columns a wave holds at a time in the backward passes: 4 registers per lane
constexpr int LINK_RANK_TILE = 16;       // queries that share one read of a candidate's row
constexpr int LINK_RANK_BLOCKS = 1024;
constexpr int LINK_MAX_D = 1024;

std::atomic<int64_t> g_link_launches[3];  // forward, backward, rank

struct LinkPartial {
  double a, b;                    // sum of w * element loss | sum of counted weights
  long long tp, fp, tn, fn, cnt;  // confusion counts | counted triples (weight pre-pass)
};

template <typename T>
__device__ __forceinline__ T link_wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void link_block_reduce_store(LinkPartial mine, LinkPartial* out) {
  __shared__ LinkPartial sh[4];
  mine.a = link_wave_sum(mine.a);
  mine.b = link_wave_sum(mine.b);
  mine.tp = link_wave_sum(mine.tp);
  mine.fp = link_wave_sum(mine.fp);
  mine.tn = link_wave_sum(mine.tn);
  mine.fn = link_wave_sum(mine.fn);
  mine.cnt = link_wave_sum(mine.cnt);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    LinkPartial t = sh[0];
    for (int w = 1; w < 4; ++w) {
      t.a += sh[w].a; t.b += sh[w].b; t.tp += sh[w].tp; t.fp += sh[w].fp; t.tn += sh[w].tn; t.fn += sh[w].fn; t.cnt += sh[w].cnt;
    }
    *out = t;
  }
}

// THE score routine: a whole wave computes sum_d a[d] r[d] b[d] in fp32.  Lane l adds its columns l, l + 64, l + 128, ... in
// ascending order as p = fma(a[d] * r[d], b[d], p); the 64 lane sums are added by the xor butterfly (32, 16, ..., 1), whose
// result is the same bits in every lane.  All 64 lanes must call it together.  Any of the rows may lie in LDS.
__device__ __forceinline__ float distmult_score(const float* a, const float* r, const float* b, int D) {
  float p = 0.0f;
  for (int d = threadIdx.x & 63; d < D; d += 64) p = fmaf(a[d] * r[d], b[d], p);
  return link_wave_sum(p);
}

__device__ __forceinline__ bool distmult_counted(float y, float w) { return w > 0.0f && (y == 0.0f || y == 1.0f); }

// Stage 0: W and the number of counted triples, one partial per workgroup.
__global__ void __launch_bounds__(256)
distmult_weight_kernel(const float* __restrict__ labels, int64_t ld_y, const float* __restrict__ weights, int64_t ld_w, int64_t N,
                       LinkPartial* __restrict__ partials) {
  LinkPartial mine = {0.0, 0.0, 0, 0, 0, 0, 0};
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (int64_t)gridDim.x * blockDim.x) {
    const float w = weights ? weights[e * ld_w] : 1.0f;
    if (distmult_counted(labels[e * ld_y], w)) {
      mine.b += (double)w;
      mine.cnt += 1;
    }
  }
  link_block_reduce_store(mine, partials + blockIdx.x);
}

// Stage 1: one wave per triple, triples to waves in a fixed grid-stride order; lane 0 carries the triple's terms.
__global__ void __launch_bounds__(256)
distmult_ce_kernel(const float* __restrict__ H, int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ triples,
                   const float* __restrict__ labels, int64_t ld_y, const float* __restrict__ weights, int64_t ld_w, int64_t N, int D,
                   const LinkPartial* __restrict__ weight_partials, int num_weight_partials, float* __restrict__ scores,
                   float* __restrict__ gscore, LinkPartial* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), num_waves = (int64_t)gridDim.x * 4;
  // every lane of every wave gets the same bits of W: the pre-pass partials, one per lane, through the fixed butterfly
  const double W = link_wave_sum(lane < num_weight_partials ? weight_partials[lane].b : 0.0);
  LinkPartial mine = {0.0, 0.0, 0, 0, 0, 0, 0};
  for (int64_t e = wave; e < N; e += num_waves) {  // wave-uniform: the shuffles need all lanes
    const int32_t u = triples[3 * e], t = triples[3 * e + 1], v = triples[3 * e + 2];
    const float s = distmult_score(H + (int64_t)u * ld_h, R + (int64_t)t * D, H + (int64_t)v * ld_h, D);
    if (lane == 0) {
      const float y = labels[e * ld_y], w = weights ? weights[e * ld_w] : 1.0f;
      float g = 0.0f;
      if (distmult_counted(y, w)) {
        mine.a += (double)w * (double)(fmaxf(s, 0.0f) - s * y + log1pf(expf(-fabsf(s))));
        const bool pred = s > 0.0f, pos = y == 1.0f;
        mine.tp += pred && pos;
        mine.fp += pred && !pos;
        mine.tn += !pred && !pos;
        mine.fn += !pred && pos;
        g = (float)((double)w / W) * (1.0f / (1.0f + expf(-s)) - y);
      }
      if (scores) scores[e] = s;
      if (gscore) gscore[e] = g;
    }
  }
  link_block_reduce_store(mine, partials + blockIdx.x);
}

// Stage 2: the partials of the main pass followed by those of the weight pre-pass, in a fixed order.
__global__ void __launch_bounds__(256)
distmult_final_kernel(const LinkPartial* __restrict__ partials, int n, float* __restrict__ metrics, long long* __restrict__ counts) {
  LinkPartial mine = {0.0, 0.0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += 256) {
    const LinkPartial p = partials[i];
    mine.a += p.a; mine.b += p.b; mine.tp += p.tp; mine.fp += p.fp; mine.tn += p.tn; mine.fn += p.fn; mine.cnt += p.cnt;
  }
  __shared__ LinkPartial total;
  link_block_reduce_store(mine, &total);
  __syncthreads();
  if (threadIdx.x == 0) {
    metrics[0] = total.cnt > 0 ? (float)(total.a / total.b) : 0.0f;
    metrics[1] = (float)((double)(total.tp + total.tn) / (double)total.cnt);  // 0 / 0 -> nan
    if (counts) { counts[0] = total.tp; counts[1] = total.fp; counts[2] = total.tn; counts[3] = total.fn; }
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------
// One list walk serves both gradients.  REL == false: `list` holds node entries 2 e + role, a term is
// g_e R[t_e, d] H[other end of e, d]; REL == true: `list` holds triple ids, a term is g_e H[u_e, d] H[v_e, d].  A wave adds
// the terms of list[begin .. end) in ascending order into the LINK_COLS columns from d0, lane l holding d0 + l + 64 k:
// acc = fma(g * x[d], y[d], acc).  The list, the triples and g are read wave-uniformly.
template <bool REL>
__device__ __forceinline__ void link_walk(const int32_t* __restrict__ list, int64_t begin, int64_t end, const float* __restrict__ H,
                                          int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ triples,
                                          const float* __restrict__ g, int D, int d0, float (&acc)[4]) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = begin; i < end; ++i) {
    const int32_t entry = list[i];
    const int64_t e = REL ? entry : (entry >> 1);
    const int32_t u = triples[3 * e], t = triples[3 * e + 1], v = triples[3 * e + 2];
    const float ge = g[e];
    const float* x = REL ? H + (int64_t)u * ld_h : R + (int64_t)t * D;
    const float* y = H + (int64_t)((!REL && (entry & 1)) ? u : v) * ld_h;  // role 1: the node is the target, the other end u
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = d0 + lane + 64 * k;
      if (d < D) acc[k] = fmaf(ge * x[d], y[d], acc[k]);
    }
  }
}

// Chunks of the long rows (more than LINK_CHUNK list positions).  Chunk k of row r covers the positions
// [offsets[r] + k CHUNK, offsets[r] + (k + 1) CHUNK) of the row.  The host cannot see which rows are long, so the grid has one
// wave ("item") per LINK_HALF list positions: item j belongs to the row that holds position j HALF, and is that row's chunk
// j - ceil(offsets[r] / HALF) if the row has that many.  A row of more than CHUNK positions holds at least floor(2 len / CHUNK)
// >= ceil(len / CHUNK) multiples of HALF, so every chunk of it finds an item.  The chunk sum goes to workspace row j.
template <bool REL>
__global__ void __launch_bounds__(256)
link_chunk_kernel(const uint32_t* __restrict__ offsets, int64_t num_rows, const int32_t* __restrict__ list, int64_t total,
                  const float* __restrict__ H, int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ triples,
                  const float* __restrict__ g, int D, float* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t pos = item * LINK_HALF;
  if (pos >= total) return;
  int64_t lo = 0, hi = num_rows - 1;  // the last row with offsets[row] <= pos: offsets[lo] <= pos throughout
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if ((int64_t)offsets[mid] <= pos) lo = mid; else hi = mid - 1;
  }
  const int64_t begin = offsets[lo], end = offsets[lo + 1];
  if (end - begin <= LINK_CHUNK) return;
  const int64_t k = item - (begin + LINK_HALF - 1) / LINK_HALF;
  const int64_t cb = begin + k * LINK_CHUNK;
  if (cb >= end) return;
  const int64_t ce = cb + LINK_CHUNK < end ? cb + LINK_CHUNK : end;
  for (int d0 = 0; d0 < D; d0 += LINK_COLS) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    link_walk<REL>(list, cb, ce, H, ld_h, R, triples, g, D, d0, acc);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int d = d0 + lane + 64 * kk;
      if (d < D) ws[item * D + d] = acc[kk];
    }
  }
}

// One wave per row (node or relation): a row of at most LINK_CHUNK positions is walked here, a longer one is the sum of its
// chunk sums in ascending chunk order.  A row without positions is written as 0.  accumulate: out = out + sum.
template <bool REL>
__global__ void __launch_bounds__(256)
link_row_kernel(const uint32_t* __restrict__ offsets, int64_t num_rows, const int32_t* __restrict__ list,
                const float* __restrict__ H, int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ triples,
                const float* __restrict__ g, int D, const float* __restrict__ ws, float* __restrict__ out, int64_t ld_out,
                int accumulate) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), num_waves = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < num_rows; r += num_waves) {
    const int64_t begin = offsets[r], end = offsets[r + 1];
    const int64_t first_item = (begin + LINK_HALF - 1) / LINK_HALF, chunks = (end - begin + LINK_CHUNK - 1) / LINK_CHUNK;
    for (int d0 = 0; d0 < D; d0 += LINK_COLS) {
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (end - begin <= LINK_CHUNK) {
        link_walk<REL>(list, begin, end, H, ld_h, R, triples, g, D, d0, acc);
      } else {
        for (int64_t k = 0; k < chunks; ++k) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const int d = d0 + lane + 64 * kk;
            if (d < D) acc[kk] += ws[(first_item + k) * D + d];
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int d = d0 + lane + 64 * kk;
        if (d < D) {
          float* o = out + r * ld_out + d;
          *o = accumulate ? *o + acc[kk] : acc[kk];
        }
      }
    }
  }
}

// ---- ranking -------------------------------------------------------------------------------------------------------------
// Pre-pass, one wave per query: the true triple's score, and MINUS the counts of the filter entries, so that the main pass,
// which counts every candidate but the true entity, leaves the filtered counts.  The filter's ids are unique per query.
__global__ void __launch_bounds__(256)
distmult_rank_true_kernel(const float* __restrict__ H, int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ queries,
                          int64_t Q, int side, const int32_t* __restrict__ filter_offsets, const int32_t* __restrict__ filter_ids,
                          int D, float* __restrict__ true_scores, int32_t* __restrict__ greater, int32_t* __restrict__ equal) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), num_waves = (int64_t)gridDim.x * 4;
  for (int64_t q = wave; q < Q; q += num_waves) {
    const int32_t u = queries[3 * q], t = queries[3 * q + 1], v = queries[3 * q + 2];
    const float* hu = H + (int64_t)u * ld_h;
    const float* rt = R + (int64_t)t * D;
    const float* hv = H + (int64_t)v * ld_h;
    const float s = distmult_score(hu, rt, hv, D);
    const int32_t truth = side == 0 ? v : u;
    int32_t gt = 0, eq = 0;
    if (filter_offsets) {
      for (int64_t i = filter_offsets[q]; i < filter_offsets[q + 1]; ++i) {
        const int32_t c = filter_ids[i];
        if (c == truth) continue;
        const float* hc = H + (int64_t)c * ld_h;
        const float sc = side == 0 ? distmult_score(hu, rt, hc, D) : distmult_score(hc, rt, hv, D);
        gt += sc > s;
        eq += sc == s;
      }
    }
    if (lane == 0) {
      true_scores[q] = s;
      greater[q] = -gt;
      equal[q] = -eq;
    }
  }
}

// Main pass.  blockIdx.y: a tile of LINK_RANK_TILE queries; the waves of blockIdx.x stride over the candidates.  A wave copies
// its candidate's row into LDS once and scores it against every query of the tile with distmult_score; its counts stay in
// registers until the end, when lane 0 adds them with integer atomics - exact in any order, so any grid is legal.
__global__ void __launch_bounds__(256)
distmult_rank_kernel(const float* __restrict__ H, int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ queries,
                     int64_t Q, int side, int64_t V, int D, const float* __restrict__ true_scores, int32_t* __restrict__ greater,
                     int32_t* __restrict__ equal) {
  __shared__ float rows[4][LINK_MAX_D];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* row = rows[w];
  const int64_t q0 = (int64_t)blockIdx.y * LINK_RANK_TILE;
  int32_t gt[LINK_RANK_TILE], eq[LINK_RANK_TILE];
#pragma unroll
  for (int i = 0; i < LINK_RANK_TILE; ++i) gt[i] = eq[i] = 0;
  for (int64_t c = (int64_t)blockIdx.x * 4 + w; c < V; c += (int64_t)gridDim.x * 4) {
    for (int d = lane; d < D; d += 64) row[d] = H[c * ld_h + d];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the row is the wave's own: written before any lane reads it
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < LINK_RANK_TILE; ++i) {
      const int64_t q = q0 + i;
      if (q < Q) {
        const int32_t u = queries[3 * q], t = queries[3 * q + 1], v = queries[3 * q + 2];
        if (c != (side == 0 ? v : u)) {
          const float* rt = R + (int64_t)t * D;
          const float sc = side == 0 ? distmult_score(H + (int64_t)u * ld_h, rt, row, D)
                                     : distmult_score(row, rt, H + (int64_t)v * ld_h, D);
          const float s = true_scores[q];
          gt[i] += sc > s;
          eq[i] += sc == s;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // and read before the next candidate overwrites it
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < LINK_RANK_TILE; ++i) {
      if (q0 + i < Q) {
        if (gt[i]) atomicAdd(greater + q0 + i, gt[i]);
        if (eq[i]) atomicAdd(equal + q0 + i, eq[i]);
      }
    }
  }
}

int64_t link_items(int64_t total) { return ceil_div(total, LINK_HALF); }

size_t backward_workspace_bytes(int64_t N, int64_t D) {
  return (size_t)(link_items(2 * N) + link_items(N)) * (size_t)D * sizeof(float);
}

}  // namespace
}  // namespace tfgnn

using namespace tfgnn;

#define TFGNN_LINK_CHECK_SIZES(name)                                                                                   \
  TFGNN_REQUIRE(D >= 1 && D <= LINK_MAX_D, name ": the width D must be in [1, %d]", LINK_MAX_D);                        \
  TFGNN_REQUIRE(V >= 1 && V < ((int64_t)1 << 31) && T >= 1 && T < ((int64_t)1 << 31), name ": V and T must be in [1, 2^31)"); \
  TFGNN_REQUIRE(ld_H >= D, name ": leading dimension of H smaller than D")

extern "C" int tfgnn_link_launch_counts(int64_t* out_counts, int n) {
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_link_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i < 3 ? g_link_launches[i].load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

extern "C" size_t tfgnn_distmult_ce_workspace_bytes(void) { return sizeof(LinkPartial) * (LINK_BLOCKS + LINK_WEIGHT_BLOCKS); }

extern "C" int tfgnn_distmult_ce_metrics(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_triples,
                                         const float* d_labels, int64_t ld_labels, const float* d_weights, int64_t ld_weights,
                                         int64_t V, int64_t T, int64_t N, int64_t D, float* d_metrics, int64_t* d_counts,
                                         float* d_scores, float* d_gscore, void* d_workspace, size_t workspace_bytes,
                                         void* stream) {
  TFGNN_REQUIRE(N >= 1, "distmult_ce_metrics: empty batch (no triple)");
  TFGNN_REQUIRE(N <= ((int64_t)1 << 30), "distmult_ce_metrics: more than 2^30 triples");
  TFGNN_LINK_CHECK_SIZES("distmult_ce_metrics");
  TFGNN_REQUIRE(d_H && d_R && d_triples && d_labels && d_metrics, "distmult_ce_metrics: NULL pointer");
  TFGNN_REQUIRE(ld_labels >= 1 && (!d_weights || ld_weights >= 1), "distmult_ce_metrics: an element stride < 1");
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= tfgnn_distmult_ce_workspace_bytes() && (uintptr_t)d_workspace % 8 == 0,
                "distmult_ce_metrics: workspace of tfgnn_distmult_ce_workspace_bytes() bytes required, 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  LinkPartial* partials = (LinkPartial*)d_workspace;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(LINK_BLOCKS, ceil_div(N, 4)));
  const int weight_grid = (int)std::max<int64_t>(1, std::min<int64_t>(LINK_WEIGHT_BLOCKS, ceil_div(N, 256 * 4)));
  LinkPartial* weight_partials = partials + grid;  // behind the main pass's: the final stage reads one array
  hipLaunchKernelGGL(distmult_weight_kernel, dim3(weight_grid), dim3(256), 0, s, d_labels, ld_labels, d_weights, ld_weights, N,
                     weight_partials);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(distmult_ce_kernel, dim3(grid), dim3(256), 0, s, d_H, ld_H, d_R, d_triples, d_labels, ld_labels, d_weights,
                     ld_weights, N, (int)D, weight_partials, weight_grid, d_scores, d_gscore, partials);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(distmult_final_kernel, dim3(1), dim3(256), 0, s, partials, grid + weight_grid, d_metrics,
                     (long long*)d_counts);
  TFGNN_LAUNCH_CHECK();
  g_link_launches[0].fetch_add(3, std::memory_order_relaxed);
  return TFGNN_OK;
}

extern "C" size_t tfgnn_distmult_backward_workspace_bytes(int64_t N, int64_t D) {
  if (N < 1 || N > ((int64_t)1 << 30) || D < 1 || D > LINK_MAX_D) return 0;
  return backward_workspace_bytes(N, D);
}

extern "C" int tfgnn_distmult_backward(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_triples,
                                       const float* d_gscore, const int32_t* d_node_offsets, const int32_t* d_node_entries,
                                       const int32_t* d_rel_offsets, const int32_t* d_rel_order, int64_t V, int64_t T, int64_t N,
                                       int64_t D, float* d_dH, int64_t ld_dH, int accumulate, float* d_dR, void* d_workspace,
                                       size_t workspace_bytes, void* stream) {
  TFGNN_REQUIRE(N >= 1, "distmult_backward: empty batch (no triple)");
  TFGNN_REQUIRE(N <= ((int64_t)1 << 30), "distmult_backward: more than 2^30 triples");
  TFGNN_LINK_CHECK_SIZES("distmult_backward");
  TFGNN_REQUIRE(d_H && d_R && d_triples && d_gscore && (d_dH || d_dR), "distmult_backward: NULL pointer");
  TFGNN_REQUIRE((!d_dH || (d_node_offsets && d_node_entries)) && (!d_dR || (d_rel_offsets && d_rel_order)),
                "distmult_backward: NULL pointer (the tables of a requested gradient)");
  TFGNN_REQUIRE(!d_dH || ld_dH >= D, "distmult_backward: leading dimension of dH smaller than D");
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= backward_workspace_bytes(N, D) && (uintptr_t)d_workspace % 4 == 0,
                "distmult_backward: workspace of tfgnn_distmult_backward_workspace_bytes(N, D) bytes required");
  hipStream_t s = (hipStream_t)stream;
  float* ws_nodes = (float*)d_workspace;
  float* ws_rels = ws_nodes + link_items(2 * N) * D;
  if (d_dH) {
    const int64_t items = link_items(2 * N);
    hipLaunchKernelGGL(link_chunk_kernel<false>, dim3((unsigned)ceil_div(items, 4)), dim3(256), 0, s, (const uint32_t*)d_node_offsets,
                       V, d_node_entries, 2 * N, d_H, ld_H, d_R, d_triples, d_gscore, (int)D, ws_nodes);
    TFGNN_LAUNCH_CHECK();
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(V, 4), 65536);
    hipLaunchKernelGGL(link_row_kernel<false>, dim3(grid), dim3(256), 0, s, (const uint32_t*)d_node_offsets, V, d_node_entries, d_H,
                       ld_H, d_R, d_triples, d_gscore, (int)D, ws_nodes, d_dH, ld_dH, accumulate);
    TFGNN_LAUNCH_CHECK();
    g_link_launches[1].fetch_add(2, std::memory_order_relaxed);
  }
  if (d_dR) {
    const int64_t items = link_items(N);
    hipLaunchKernelGGL(link_chunk_kernel<true>, dim3((unsigned)ceil_div(items, 4)), dim3(256), 0, s, (const uint32_t*)d_rel_offsets, T,
                       d_rel_order, N, d_H, ld_H, d_R, d_triples, d_gscore, (int)D, ws_rels);
    TFGNN_LAUNCH_CHECK();
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(T, 4), 65536);
    hipLaunchKernelGGL(link_row_kernel<true>, dim3(grid), dim3(256), 0, s, (const uint32_t*)d_rel_offsets, T, d_rel_order, d_H, ld_H,
                       d_R, d_triples, d_gscore, (int)D, ws_rels, d_dR, D, 0);
    TFGNN_LAUNCH_CHECK();
    g_link_launches[1].fetch_add(2, std::memory_order_relaxed);
  }
  return TFGNN_OK;
}

extern "C" size_t tfgnn_distmult_rank_workspace_bytes(int64_t Q) { return Q < 1 ? 0 : (size_t)Q * sizeof(float); }

extern "C" int tfgnn_distmult_rank(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_queries, int64_t Q, int side,
                                   const int32_t* d_filter_offsets, const int32_t* d_filter_ids, int64_t V, int64_t T, int64_t D,
                                   int32_t* d_greater, int32_t* d_equal, void* d_workspace, size_t workspace_bytes, void* stream) {
  TFGNN_REQUIRE(Q >= 1, "distmult_rank: empty batch (no query)");
  TFGNN_REQUIRE(Q <= ((int64_t)1 << 30), "distmult_rank: more than 2^30 queries");
  TFGNN_REQUIRE(side == 0 || side == 1, "distmult_rank: side must be 0 (corrupt the target) or 1 (corrupt the source)");
  TFGNN_LINK_CHECK_SIZES("distmult_rank");
  TFGNN_REQUIRE(d_H && d_R && d_queries && d_greater && d_equal, "distmult_rank: NULL pointer");
  TFGNN_REQUIRE((d_filter_offsets == nullptr) == (d_filter_ids == nullptr), "distmult_rank: a filter needs both its offsets and its ids");
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= tfgnn_distmult_rank_workspace_bytes(Q) && (uintptr_t)d_workspace % 4 == 0,
                "distmult_rank: workspace of tfgnn_distmult_rank_workspace_bytes(Q) bytes required");
  hipStream_t s = (hipStream_t)stream;
  float* true_scores = (float*)d_workspace;
  const unsigned pre_grid = (unsigned)std::min<int64_t>(ceil_div(Q, 4), LINK_RANK_BLOCKS);
  hipLaunchKernelGGL(distmult_rank_true_kernel, dim3(pre_grid), dim3(256), 0, s, d_H, ld_H, d_R, d_queries, Q, side, d_filter_offsets,
                     d_filter_ids, (int)D, true_scores, d_greater, d_equal);
  TFGNN_LAUNCH_CHECK();
  const int64_t tiles = ceil_div(Q, LINK_RANK_TILE);
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(V, 4), LINK_RANK_BLOCKS);
  for (int64_t t0 = 0; t0 < tiles; t0 += 65535) {  // blockIdx.y is limited to 65535 tiles per launch
    const int64_t nt = std::min<int64_t>(65535, tiles - t0);
    const int64_t qoff = t0 * LINK_RANK_TILE;
    hipLaunchKernelGGL(distmult_rank_kernel, dim3(gx, (unsigned)nt), dim3(256), 0, s, d_H, ld_H, d_R, d_queries + 3 * qoff, Q - qoff,
                       side, V, (int)D, true_scores + qoff, d_greater + qoff, d_equal + qoff);
    TFGNN_LAUNCH_CHECK();
    g_link_launches[2].fetch_add(1, std::memory_order_relaxed);
  }
  g_link_launches[2].fetch_add(1, std::memory_order_relaxed);
  return TFGNN_OK;
}
