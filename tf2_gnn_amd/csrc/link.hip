// Link prediction decoders (LinkPredictionTask; the reference has no counterpart, PARITY UNPINNED): the score of a typed edge
// (u, t, v) from the final node representations.  DistMult: s = sum_d H[u, d] R[t, d] H[v, d].  ComplEx: a row is the complex
// vector [re ; im] (halves), s = Re sum_k H[u, k] R[t, k] conj(H[v, k]); the tfgnn_complex_* calls mirror the three below.
//   tfgnn_distmult_ce_metrics: scores, weighted sigmoid cross-entropy, confusion counts, d loss / d score
//   tfgnn_distmult_backward:   d loss / d H (a CSR row walk over the triples of every node) and d loss / d R (over the triples
//                              of every relation)
//   tfgnn_distmult_rank:       for evaluation, how many candidate entities score above / equal to the true one
// The contracts are the comments in include/tfgnn.h.  Every DistMult score of every kernel comes out of distmult_score below,
// every ComplEx score out of complex_score (training) or complex_dot (ranking: query vector times candidate row).  The loss,
// the table walk and the host checks exist once, as templates over the decoder (DEC: LINK_DISTMULT / LINK_COMPLEX).  No
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
constexpr int LINK_COLS = 256;           // columns a wave holds at a time in the backward passes: 4 registers per lane (ComplEx:
                                         // complex columns, 4 for the re and 4 for the im parts)
constexpr int LINK_RANK_TILE = 16;       // queries that share one read of a candidate's row
constexpr int LINK_RANK_BLOCKS = 1024;
constexpr int LINK_MAX_D = 1024;

constexpr int LINK_DISTMULT = 0, LINK_COMPLEX = 1;  // the DEC template argument

std::atomic<int64_t> g_link_launches[2][3];  // [decoder][forward, backward, rank]

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

// THE ComplEx score routine: Re sum_k a[k] r[k] conj(b[k]) over the m = D / 2 complex columns, x[k] = x[k] + i x[m + k].  Lane l
// adds its columns k = l, l + 64, ... in ascending order; per column
//   x = fma(a_im, b_im, a_re * b_re),  y = fma(-a_im, b_re, a_re * b_im),  p = fma(r_re, x, p),  p = fma(r_im, y, p)
// and the 64 lane sums go through the same butterfly.  All 64 lanes must call it together.
__device__ __forceinline__ float complex_score(const float* a, const float* r, const float* b, int D) {
  const int m = D >> 1;
  float p = 0.0f;
  for (int k = threadIdx.x & 63; k < m; k += 64) {
    const float are = a[k], aim = a[m + k], bre = b[k], bim = b[m + k];
    const float x = fmaf(aim, bim, are * bre), y = fmaf(-aim, bre, are * bim);
    p = fmaf(r[k], x, p);
    p = fmaf(r[m + k], y, p);
  }
  return link_wave_sum(p);
}

// The score of the ComplEx ranking call: the plain D-long dot product of a query vector (complex_query) with a candidate's
// row, lane l adding d = l, l + 64, ... in ascending order as p = fma(q[d], c[d], p), then the butterfly.
__device__ __forceinline__ float complex_dot(const float* q, const float* c, int D) {
  float p = 0.0f;
  for (int d = threadIdx.x & 63; d < D; d += 64) p = fmaf(q[d], c[d], p);
  return link_wave_sum(p);
}

// The query vector of a ranking query, written by the whole wave: s(u, t, c) = <q, H[c]> for side 0 (x = H[u]),
//   q_re = fma(r_re, x_re, -(r_im * x_im)),  q_im = fma(r_re, x_im, r_im * x_re);
// s(c, t, v) = <q', H[c]> for side 1 (x = H[v]):  q'_re = fma(r_re, x_re, r_im * x_im),  q'_im = fma(r_re, x_im, -(r_im * x_re)).
__device__ __forceinline__ void complex_query(const float* x, const float* r, int side, int D, float* q) {
  const int m = D >> 1;
  for (int k = threadIdx.x & 63; k < m; k += 64) {
    const float xre = x[k], xim = x[m + k], rre = r[k], rim = r[m + k];
    const float sim = side == 0 ? rim : -rim;
    q[k] = fmaf(rre, xre, -(sim * xim));
    q[m + k] = fmaf(rre, xim, sim * xre);
  }
}

template <int DEC>
__device__ __forceinline__ float link_score(const float* a, const float* r, const float* b, int D) {
  if constexpr (DEC == LINK_COMPLEX) return complex_score(a, r, b, D);
  else return distmult_score(a, r, b, D);
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
template <int DEC>
__global__ void __launch_bounds__(256)
link_ce_kernel(const float* __restrict__ H, int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ triples,
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
    const float s = link_score<DEC>(H + (int64_t)u * ld_h, R + (int64_t)t * D, H + (int64_t)v * ld_h, D);
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
//
// ComplEx (DEC == LINK_COMPLEX): the wave holds LINK_COLS COMPLEX columns from d0, lane l the columns c = d0 + l + 64 k with
// re in acc[k] and im in acc[4 + k], so the four row reads of a term (x_re, x_im, y_re, y_im) are made once for both parts.
// With (x, y) as above, gr = g * x_re, gi = g * x_im and sg = -gi when the node is the target (role 1), else gi:
//   acc_re = fma(gr, y_re, acc_re);  acc_re = fma(sg, y_im, acc_re);  acc_im = fma(gr, y_im, acc_im);  acc_im = fma(-sg, y_re, acc_im)
// which is d s / d a (role 0), d s / d b (role 1) and d s / d r (REL) of s = Re sum a r conj(b), each times g.
template <int DEC>
constexpr int link_slots() { return DEC == LINK_COMPLEX ? 8 : 4; }  // accumulators per lane

// The columns the d0 loop of a wave runs over: float columns (DistMult) or complex columns (ComplEx).
template <int DEC>
__device__ __forceinline__ int link_span(int D) { return DEC == LINK_COMPLEX ? (D >> 1) : D; }

// The float column of accumulator k of this lane -> d; false when it lies outside the row.
template <int DEC>
__device__ __forceinline__ bool link_slot_col(int d0, int lane, int k, int D, int& d) {
  if constexpr (DEC == LINK_COMPLEX) {
    const int m = D >> 1, c = d0 + lane + 64 * (k & 3);
    d = c + (k >> 2) * m;
    return c < m;
  } else {
    d = d0 + lane + 64 * k;
    return d < D;
  }
}

template <bool REL, int DEC>
__device__ __forceinline__ void link_walk(const int32_t* __restrict__ list, int64_t begin, int64_t end, const float* __restrict__ H,
                                          int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ triples,
                                          const float* __restrict__ g, int D, int d0, float (&acc)[link_slots<DEC>()]) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = begin; i < end; ++i) {
    const int32_t entry = list[i];
    const int64_t e = REL ? entry : (entry >> 1);
    const int32_t u = triples[3 * e], t = triples[3 * e + 1], v = triples[3 * e + 2];
    const float ge = g[e];
    const float* x = REL ? H + (int64_t)u * ld_h : R + (int64_t)t * D;
    const float* y = H + (int64_t)((!REL && (entry & 1)) ? u : v) * ld_h;  // role 1: the node is the target, the other end u
    if constexpr (DEC == LINK_COMPLEX) {
      const int m = D >> 1;
      const bool target = !REL && (entry & 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = d0 + lane + 64 * k;
        if (c < m) {
          const float yre = y[c], yim = y[m + c];
          const float gr = ge * x[c], gi = ge * x[m + c];
          const float sg = target ? -gi : gi;
          acc[k] = fmaf(gr, yre, acc[k]);
          acc[k] = fmaf(sg, yim, acc[k]);
          acc[4 + k] = fmaf(gr, yim, acc[4 + k]);
          acc[4 + k] = fmaf(-sg, yre, acc[4 + k]);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int d = d0 + lane + 64 * k;
        if (d < D) acc[k] = fmaf(ge * x[d], y[d], acc[k]);
      }
    }
  }
}

// Chunks of the long rows (more than LINK_CHUNK list positions).  Chunk k of row r covers the positions
// [offsets[r] + k CHUNK, offsets[r] + (k + 1) CHUNK) of the row.  The host cannot see which rows are long, so the grid has one
// wave ("item") per LINK_HALF list positions: item j belongs to the row that holds position j HALF, and is that row's chunk
// j - ceil(offsets[r] / HALF) if the row has that many.  A row of more than CHUNK positions holds at least floor(2 len / CHUNK)
// >= ceil(len / CHUNK) multiples of HALF, so every chunk of it finds an item.  The chunk sum goes to workspace row j.
template <bool REL, int DEC>
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
  for (int d0 = 0; d0 < link_span<DEC>(D); d0 += LINK_COLS) {
    float acc[link_slots<DEC>()] = {};
    link_walk<REL, DEC>(list, cb, ce, H, ld_h, R, triples, g, D, d0, acc);
#pragma unroll
    for (int kk = 0; kk < link_slots<DEC>(); ++kk) {
      int d;
      if (link_slot_col<DEC>(d0, lane, kk, D, d)) ws[item * D + d] = acc[kk];
    }
  }
}

// One wave per row (node or relation): a row of at most LINK_CHUNK positions is walked here, a longer one is the sum of its
// chunk sums in ascending chunk order.  A row without positions is written as 0.  accumulate: out = out + sum.
template <bool REL, int DEC>
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
    for (int d0 = 0; d0 < link_span<DEC>(D); d0 += LINK_COLS) {
      float acc[link_slots<DEC>()] = {};
      if (end - begin <= LINK_CHUNK) {
        link_walk<REL, DEC>(list, begin, end, H, ld_h, R, triples, g, D, d0, acc);
      } else {
        for (int64_t k = 0; k < chunks; ++k) {
#pragma unroll
          for (int kk = 0; kk < link_slots<DEC>(); ++kk) {
            int d;
            if (link_slot_col<DEC>(d0, lane, kk, D, d)) acc[kk] += ws[(first_item + k) * D + d];
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < link_slots<DEC>(); ++kk) {
        int d;
        if (link_slot_col<DEC>(d0, lane, kk, D, d)) {
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

// ComplEx pre-pass, one wave per query: the query vector goes to LDS (for this wave's own scores) and to qvec [Q, D] (for
// the main pass).  Every score of the call - the true triple's, the filter ids', the candidates' - is complex_dot of that
// vector with a node's row, so a row equal to the true entity's bit for bit scores equal.
__global__ void __launch_bounds__(256)
complex_rank_true_kernel(const float* __restrict__ H, int64_t ld_h, const float* __restrict__ R, const int32_t* __restrict__ queries,
                         int64_t Q, int side, const int32_t* __restrict__ filter_offsets, const int32_t* __restrict__ filter_ids,
                         int D, float* __restrict__ qvec, float* __restrict__ true_scores, int32_t* __restrict__ greater,
                         int32_t* __restrict__ equal) {
  __shared__ float qs[4][LINK_MAX_D];
  const int lane = threadIdx.x & 63;
  float* q_lds = qs[threadIdx.x >> 6];
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), num_waves = (int64_t)gridDim.x * 4;
  for (int64_t q = wave; q < Q; q += num_waves) {
    const int32_t u = queries[3 * q], t = queries[3 * q + 1], v = queries[3 * q + 2];
    const int32_t truth = side == 0 ? v : u;
    complex_query(H + (int64_t)(side == 0 ? u : v) * ld_h, R + (int64_t)t * D, side, D, q_lds);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the vector is the wave's own: written before any lane reads it
    __builtin_amdgcn_wave_barrier();
    for (int d = lane; d < D; d += 64) qvec[q * D + d] = q_lds[d];
    const float s = complex_dot(q_lds, H + (int64_t)truth * ld_h, D);
    int32_t gt = 0, eq = 0;
    if (filter_offsets) {
      for (int64_t i = filter_offsets[q]; i < filter_offsets[q + 1]; ++i) {
        const int32_t c = filter_ids[i];
        if (c == truth) continue;
        const float sc = complex_dot(q_lds, H + (int64_t)c * ld_h, D);
        gt += sc > s;
        eq += sc == s;
      }
    }
    if (lane == 0) {
      true_scores[q] = s;
      greater[q] = -gt;
      equal[q] = -eq;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // and read before the next query overwrites it
    __builtin_amdgcn_wave_barrier();
  }
}

// ComplEx main pass: the grid and the counting of distmult_rank_kernel; a score is complex_dot of the query's vector with the
// LDS-resident candidate row.  Held to 5 waves per SIMD (95 registers, no scratch): left alone the compiler takes 123 registers
// for the 16 unrolled dot products and the pass, which is bound by latency, measured 19 % slower; 6 waves would spill.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5)))
complex_rank_kernel(const float* __restrict__ H, int64_t ld_h, const int32_t* __restrict__ queries, int64_t Q, int side, int64_t V,
                    int D, const float* __restrict__ qvec, const float* __restrict__ true_scores, int32_t* __restrict__ greater,
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
        if (c != queries[3 * q + (side == 0 ? 2 : 0)]) {
          const float sc = complex_dot(qvec + q * D, row, D);
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

constexpr const char* LINK_NAMES[2] = {"distmult", "complex"};

// The size rules the three calls of a decoder share, as one expression per message.
#define TFGNN_LINK_CHECK_SIZES(call)                                                                                          \
  TFGNN_REQUIRE(D >= (DEC == LINK_COMPLEX ? 2 : 1) && D <= LINK_MAX_D, "%s_" call ": the width D must be in [%d, %d]",        \
                LINK_NAMES[DEC], DEC == LINK_COMPLEX ? 2 : 1, LINK_MAX_D);                                                     \
  TFGNN_REQUIRE(DEC != LINK_COMPLEX || D % 2 == 0, "%s_" call ": the width D must be even (re and im halves)", LINK_NAMES[DEC]); \
  TFGNN_REQUIRE(V >= 1 && V < ((int64_t)1 << 31) && T >= 1 && T < ((int64_t)1 << 31), "%s_" call ": V and T must be in [1, 2^31)", \
                LINK_NAMES[DEC]);                                                                                             \
  TFGNN_REQUIRE(ld_H >= D, "%s_" call ": leading dimension of H smaller than D", LINK_NAMES[DEC])

bool link_width_ok(int dec, int64_t D) { return dec == LINK_COMPLEX ? (D >= 2 && D <= LINK_MAX_D && D % 2 == 0) : (D >= 1 && D <= LINK_MAX_D); }

size_t ce_workspace_bytes() { return sizeof(LinkPartial) * (LINK_BLOCKS + LINK_WEIGHT_BLOCKS); }

template <int DEC>
int link_ce_metrics(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_triples, const float* d_labels,
                    int64_t ld_labels, const float* d_weights, int64_t ld_weights, int64_t V, int64_t T, int64_t N, int64_t D,
                    float* d_metrics, int64_t* d_counts, float* d_scores, float* d_gscore, void* d_workspace, size_t workspace_bytes,
                    void* stream) {
  const char* name = LINK_NAMES[DEC];
  TFGNN_REQUIRE(N >= 1, "%s_ce_metrics: empty batch (no triple)", name);
  TFGNN_REQUIRE(N <= ((int64_t)1 << 30), "%s_ce_metrics: more than 2^30 triples", name);
  TFGNN_LINK_CHECK_SIZES("ce_metrics");
  TFGNN_REQUIRE(d_H && d_R && d_triples && d_labels && d_metrics, "%s_ce_metrics: NULL pointer", name);
  TFGNN_REQUIRE(ld_labels >= 1 && (!d_weights || ld_weights >= 1), "%s_ce_metrics: an element stride < 1", name);
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= ce_workspace_bytes() && (uintptr_t)d_workspace % 8 == 0,
                "%s_ce_metrics: workspace of tfgnn_%s_ce_workspace_bytes() bytes required, 8-byte aligned", name, name);
  hipStream_t s = (hipStream_t)stream;
  LinkPartial* partials = (LinkPartial*)d_workspace;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(LINK_BLOCKS, ceil_div(N, 4)));
  const int weight_grid = (int)std::max<int64_t>(1, std::min<int64_t>(LINK_WEIGHT_BLOCKS, ceil_div(N, 256 * 4)));
  LinkPartial* weight_partials = partials + grid;  // behind the main pass's: the final stage reads one array
  hipLaunchKernelGGL(distmult_weight_kernel, dim3(weight_grid), dim3(256), 0, s, d_labels, ld_labels, d_weights, ld_weights, N,
                     weight_partials);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(link_ce_kernel<DEC>, dim3(grid), dim3(256), 0, s, d_H, ld_H, d_R, d_triples, d_labels, ld_labels, d_weights,
                     ld_weights, N, (int)D, weight_partials, weight_grid, d_scores, d_gscore, partials);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(distmult_final_kernel, dim3(1), dim3(256), 0, s, partials, grid + weight_grid, d_metrics,
                     (long long*)d_counts);
  TFGNN_LAUNCH_CHECK();
  g_link_launches[DEC][0].fetch_add(3, std::memory_order_relaxed);
  return TFGNN_OK;
}

template <int DEC>
int link_backward(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_triples, const float* d_gscore,
                  const int32_t* d_node_offsets, const int32_t* d_node_entries, const int32_t* d_rel_offsets,
                  const int32_t* d_rel_order, int64_t V, int64_t T, int64_t N, int64_t D, float* d_dH, int64_t ld_dH, int accumulate,
                  float* d_dR, void* d_workspace, size_t workspace_bytes, void* stream) {
  const char* name = LINK_NAMES[DEC];
  TFGNN_REQUIRE(N >= 1, "%s_backward: empty batch (no triple)", name);
  TFGNN_REQUIRE(N <= ((int64_t)1 << 30), "%s_backward: more than 2^30 triples", name);
  TFGNN_LINK_CHECK_SIZES("backward");
  TFGNN_REQUIRE(d_H && d_R && d_triples && d_gscore && (d_dH || d_dR), "%s_backward: NULL pointer", name);
  TFGNN_REQUIRE((!d_dH || (d_node_offsets && d_node_entries)) && (!d_dR || (d_rel_offsets && d_rel_order)),
                "%s_backward: NULL pointer (the tables of a requested gradient)", name);
  TFGNN_REQUIRE(!d_dH || ld_dH >= D, "%s_backward: leading dimension of dH smaller than D", name);
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= backward_workspace_bytes(N, D) && (uintptr_t)d_workspace % 4 == 0,
                "%s_backward: workspace of tfgnn_%s_backward_workspace_bytes(N, D) bytes required", name, name);
  hipStream_t s = (hipStream_t)stream;
  float* ws_nodes = (float*)d_workspace;
  float* ws_rels = ws_nodes + link_items(2 * N) * D;
  if (d_dH) {
    const int64_t items = link_items(2 * N);
    hipLaunchKernelGGL((link_chunk_kernel<false, DEC>), dim3((unsigned)ceil_div(items, 4)), dim3(256), 0, s,
                       (const uint32_t*)d_node_offsets, V, d_node_entries, 2 * N, d_H, ld_H, d_R, d_triples, d_gscore, (int)D, ws_nodes);
    TFGNN_LAUNCH_CHECK();
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(V, 4), 65536);
    hipLaunchKernelGGL((link_row_kernel<false, DEC>), dim3(grid), dim3(256), 0, s, (const uint32_t*)d_node_offsets, V, d_node_entries,
                       d_H, ld_H, d_R, d_triples, d_gscore, (int)D, ws_nodes, d_dH, ld_dH, accumulate);
    TFGNN_LAUNCH_CHECK();
    g_link_launches[DEC][1].fetch_add(2, std::memory_order_relaxed);
  }
  if (d_dR) {
    const int64_t items = link_items(N);
    hipLaunchKernelGGL((link_chunk_kernel<true, DEC>), dim3((unsigned)ceil_div(items, 4)), dim3(256), 0, s,
                       (const uint32_t*)d_rel_offsets, T, d_rel_order, N, d_H, ld_H, d_R, d_triples, d_gscore, (int)D, ws_rels);
    TFGNN_LAUNCH_CHECK();
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(T, 4), 65536);
    hipLaunchKernelGGL((link_row_kernel<true, DEC>), dim3(grid), dim3(256), 0, s, (const uint32_t*)d_rel_offsets, T, d_rel_order, d_H,
                       ld_H, d_R, d_triples, d_gscore, (int)D, ws_rels, d_dR, D, 0);
    TFGNN_LAUNCH_CHECK();
    g_link_launches[DEC][1].fetch_add(2, std::memory_order_relaxed);
  }
  return TFGNN_OK;
}

// DistMult: the true scores [Q].  ComplEx: the query vectors [Q, D], then the true scores [Q].
size_t rank_workspace_bytes(int dec, int64_t Q, int64_t D) {
  return (size_t)Q * (size_t)(dec == LINK_COMPLEX ? D + 1 : 1) * sizeof(float);
}

template <int DEC>
int link_rank(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_queries, int64_t Q, int side,
              const int32_t* d_filter_offsets, const int32_t* d_filter_ids, int64_t V, int64_t T, int64_t D, int32_t* d_greater,
              int32_t* d_equal, void* d_workspace, size_t workspace_bytes, void* stream) {
  const char* name = LINK_NAMES[DEC];
  TFGNN_REQUIRE(Q >= 1, "%s_rank: empty batch (no query)", name);
  TFGNN_REQUIRE(Q <= ((int64_t)1 << 30), "%s_rank: more than 2^30 queries", name);
  TFGNN_REQUIRE(side == 0 || side == 1, "%s_rank: side must be 0 (corrupt the target) or 1 (corrupt the source)", name);
  TFGNN_LINK_CHECK_SIZES("rank");
  TFGNN_REQUIRE(d_H && d_R && d_queries && d_greater && d_equal, "%s_rank: NULL pointer", name);
  TFGNN_REQUIRE((d_filter_offsets == nullptr) == (d_filter_ids == nullptr), "%s_rank: a filter needs both its offsets and its ids",
                name);
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= rank_workspace_bytes(DEC, Q, D) && (uintptr_t)d_workspace % 4 == 0,
                "%s_rank: workspace of tfgnn_%s_rank_workspace_bytes bytes required", name, name);
  hipStream_t s = (hipStream_t)stream;
  float* qvec = (float*)d_workspace;  // ComplEx only
  float* true_scores = DEC == LINK_COMPLEX ? qvec + Q * D : (float*)d_workspace;
  const unsigned pre_grid = (unsigned)std::min<int64_t>(ceil_div(Q, 4), LINK_RANK_BLOCKS);
  if constexpr (DEC == LINK_COMPLEX) {
    hipLaunchKernelGGL(complex_rank_true_kernel, dim3(pre_grid), dim3(256), 0, s, d_H, ld_H, d_R, d_queries, Q, side, d_filter_offsets,
                       d_filter_ids, (int)D, qvec, true_scores, d_greater, d_equal);
  } else {
    hipLaunchKernelGGL(distmult_rank_true_kernel, dim3(pre_grid), dim3(256), 0, s, d_H, ld_H, d_R, d_queries, Q, side, d_filter_offsets,
                       d_filter_ids, (int)D, true_scores, d_greater, d_equal);
  }
  TFGNN_LAUNCH_CHECK();
  const int64_t tiles = ceil_div(Q, LINK_RANK_TILE);
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(V, 4), LINK_RANK_BLOCKS);
  for (int64_t t0 = 0; t0 < tiles; t0 += 65535) {  // blockIdx.y is limited to 65535 tiles per launch
    const int64_t nt = std::min<int64_t>(65535, tiles - t0);
    const int64_t qoff = t0 * LINK_RANK_TILE;
    if constexpr (DEC == LINK_COMPLEX) {
      hipLaunchKernelGGL(complex_rank_kernel, dim3(gx, (unsigned)nt), dim3(256), 0, s, d_H, ld_H, d_queries + 3 * qoff, Q - qoff, side,
                         V, (int)D, qvec + qoff * D, true_scores + qoff, d_greater + qoff, d_equal + qoff);
    } else {
      hipLaunchKernelGGL(distmult_rank_kernel, dim3(gx, (unsigned)nt), dim3(256), 0, s, d_H, ld_H, d_R, d_queries + 3 * qoff, Q - qoff,
                         side, V, (int)D, true_scores + qoff, d_greater + qoff, d_equal + qoff);
    }
    TFGNN_LAUNCH_CHECK();
    g_link_launches[DEC][2].fetch_add(1, std::memory_order_relaxed);
  }
  g_link_launches[DEC][2].fetch_add(1, std::memory_order_relaxed);
  return TFGNN_OK;
}

int link_launch_counts(int dec, const char* name, int64_t* out_counts, int n) {
  TFGNN_REQUIRE(out_counts && n >= 0, "%s: bad argument", name);
  for (int i = 0; i < n; ++i) out_counts[i] = i < 3 ? g_link_launches[dec][i].load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

}  // namespace
}  // namespace tfgnn

using namespace tfgnn;

// The two decoders' entries: the same argument lists, one implementation each above.
#define TFGNN_LINK_CE_ARGS                                                                                                     \
  const float *d_H, int64_t ld_H, const float *d_R, const int32_t *d_triples, const float *d_labels, int64_t ld_labels,        \
      const float *d_weights, int64_t ld_weights, int64_t V, int64_t T, int64_t N, int64_t D, float *d_metrics, int64_t *d_counts, \
      float *d_scores, float *d_gscore, void *d_workspace, size_t workspace_bytes, void *stream
#define TFGNN_LINK_CE_PASS                                                                                                     \
  d_H, ld_H, d_R, d_triples, d_labels, ld_labels, d_weights, ld_weights, V, T, N, D, d_metrics, d_counts, d_scores, d_gscore,   \
      d_workspace, workspace_bytes, stream
#define TFGNN_LINK_BWD_ARGS                                                                                                    \
  const float *d_H, int64_t ld_H, const float *d_R, const int32_t *d_triples, const float *d_gscore,                           \
      const int32_t *d_node_offsets, const int32_t *d_node_entries, const int32_t *d_rel_offsets, const int32_t *d_rel_order,  \
      int64_t V, int64_t T, int64_t N, int64_t D, float *d_dH, int64_t ld_dH, int accumulate, float *d_dR, void *d_workspace,  \
      size_t workspace_bytes, void *stream
#define TFGNN_LINK_BWD_PASS                                                                                                    \
  d_H, ld_H, d_R, d_triples, d_gscore, d_node_offsets, d_node_entries, d_rel_offsets, d_rel_order, V, T, N, D, d_dH, ld_dH,     \
      accumulate, d_dR, d_workspace, workspace_bytes, stream
#define TFGNN_LINK_RANK_ARGS                                                                                                   \
  const float *d_H, int64_t ld_H, const float *d_R, const int32_t *d_queries, int64_t Q, int side,                             \
      const int32_t *d_filter_offsets, const int32_t *d_filter_ids, int64_t V, int64_t T, int64_t D, int32_t *d_greater,       \
      int32_t *d_equal, void *d_workspace, size_t workspace_bytes, void *stream
#define TFGNN_LINK_RANK_PASS                                                                                                   \
  d_H, ld_H, d_R, d_queries, Q, side, d_filter_offsets, d_filter_ids, V, T, D, d_greater, d_equal, d_workspace, workspace_bytes, \
      stream

extern "C" int tfgnn_link_launch_counts(int64_t* out_counts, int n) {
  return link_launch_counts(LINK_DISTMULT, "tfgnn_link_launch_counts", out_counts, n);
}
extern "C" size_t tfgnn_distmult_ce_workspace_bytes(void) { return ce_workspace_bytes(); }
extern "C" int tfgnn_distmult_ce_metrics(TFGNN_LINK_CE_ARGS) { return link_ce_metrics<LINK_DISTMULT>(TFGNN_LINK_CE_PASS); }
extern "C" size_t tfgnn_distmult_backward_workspace_bytes(int64_t N, int64_t D) {
  if (N < 1 || N > ((int64_t)1 << 30) || !link_width_ok(LINK_DISTMULT, D)) return 0;
  return backward_workspace_bytes(N, D);
}
extern "C" int tfgnn_distmult_backward(TFGNN_LINK_BWD_ARGS) { return link_backward<LINK_DISTMULT>(TFGNN_LINK_BWD_PASS); }
extern "C" size_t tfgnn_distmult_rank_workspace_bytes(int64_t Q) { return Q < 1 ? 0 : rank_workspace_bytes(LINK_DISTMULT, Q, 1); }
extern "C" int tfgnn_distmult_rank(TFGNN_LINK_RANK_ARGS) { return link_rank<LINK_DISTMULT>(TFGNN_LINK_RANK_PASS); }

extern "C" int tfgnn_complex_launch_counts(int64_t* out_counts, int n) {
  return link_launch_counts(LINK_COMPLEX, "tfgnn_complex_launch_counts", out_counts, n);
}
extern "C" size_t tfgnn_complex_ce_workspace_bytes(void) { return ce_workspace_bytes(); }
extern "C" int tfgnn_complex_ce_metrics(TFGNN_LINK_CE_ARGS) { return link_ce_metrics<LINK_COMPLEX>(TFGNN_LINK_CE_PASS); }
extern "C" size_t tfgnn_complex_backward_workspace_bytes(int64_t N, int64_t D) {
  if (N < 1 || N > ((int64_t)1 << 30) || !link_width_ok(LINK_COMPLEX, D)) return 0;
  return backward_workspace_bytes(N, D);
}
extern "C" int tfgnn_complex_backward(TFGNN_LINK_BWD_ARGS) { return link_backward<LINK_COMPLEX>(TFGNN_LINK_BWD_PASS); }
extern "C" size_t tfgnn_complex_rank_workspace_bytes(int64_t Q, int64_t D) {
  if (Q < 1 || Q > ((int64_t)1 << 30) || !link_width_ok(LINK_COMPLEX, D)) return 0;
  return rank_workspace_bytes(LINK_COMPLEX, Q, D);
}
extern "C" int tfgnn_complex_rank(TFGNN_LINK_RANK_ARGS) { return link_rank<LINK_COMPLEX>(TFGNN_LINK_RANK_PASS); }
