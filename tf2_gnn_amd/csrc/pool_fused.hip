// Graph readout in one forward and one backward call (tfgnn_pool_forward / tfgnn_pool_backward, include/tfgnn.h):
// the tail of WeightedSumGraphRepresentation.call (tf2_gnn/layers/nodes_to_graph_representation.py:170-229) behind the two
// MLPs - per-graph softmax of the scores, clip of the transformed nodes, weighted segment sum - and its gradient.
//
// Mapping (DESIGN.md "Graph readout"): the nodes are cut into tiles of kChunk nodes, one 256-thread workgroup per tile.
// A tile OWNS the graphs whose first node lies in it and, of a graph of more than kChunk nodes, the chunk
// [beg + k * kChunk, beg + (k + 1) * kChunk) whose first node lies in it - at most one chunk of a graph that began earlier
// (slot 0) and the first chunk of a large graph that begins here (slot 1).  Each owned segment is reduced by ONE wave, the
// four waves of the workgroup take the tile's segments round-robin; inside the wave the lanes are spread over
// (nodes x features): CL lanes along the features (float4 each when the rows allow), 64 / CL lanes along the nodes.
// Graphs of at most kChunk nodes are finished by their wave.  Chunks of larger graphs leave partial results in the caller's
// workspace (running max, sum of exponentials, weighted sums, sum of w * dw) and a second launch combines them chunk by
// chunk in ascending order.  Every sum has a fixed shape that depends on kChunk and the graph alone: no atomics, and the
// result does not change with the grid, the device or the run.
#include <atomic>
#include <cmath>

#include "common.hpp"

namespace tfgnn {

constexpr int kChunk = TFGNN_POOL_CHUNK_NODES;
constexpr int kPoolMaxWidth = 1024;  // widest row whose per-wave staging fits the 64 KiB of LDS a launch may ask for

static std::atomic<int64_t> g_pool_launches[2];

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// first index in [0, n) with ptr[index] >= val, n when there is none
__device__ __forceinline__ int ptr_lower_bound(const int32_t* __restrict__ ptr, int n, int val) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] < val) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct PoolSeg {
  int g, beg, end;  // graph, node range of the segment
  int gbeg, gend;   // node range of the whole graph
  int slot;         // -1: the whole graph; 0 / 1: a chunk of a larger graph, partial results go to this slot of the tile
};

struct PoolTile {
  int gA, gB;       // graphs [gA, gB) begin in this tile
  int has_chunk;    // a graph that began earlier has a chunk beginning here
  PoolSeg chunk;
  int V;
  const int32_t* ptr;

  __device__ __forceinline__ int num_segments() const { return has_chunk + (gB - gA); }
  __device__ __forceinline__ PoolSeg segment(int i) const {
    if (has_chunk) {
      if (i == 0) return chunk;
      --i;
    }
    PoolSeg s;
    s.g = gA + i;
    s.gbeg = min(ptr[s.g], V);
    s.gend = min(max(ptr[s.g + 1], s.gbeg), V);
    s.beg = s.gbeg;
    s.end = s.gend;
    s.slot = -1;
    if (s.gend - s.gbeg > kChunk) {
      s.end = s.gbeg + kChunk;
      s.slot = 1;
    }
    return s;
  }
};

__device__ __forceinline__ PoolTile pool_tile(const int32_t* __restrict__ ptr, int V, int G, int tile, int ntiles) {
  PoolTile t;
  t.ptr = ptr;
  t.V = V;
  const int n0 = tile * kChunk;
  const int n1 = min(n0 + kChunk, V);
  t.gA = min(ptr_lower_bound(ptr, G + 1, n0), G);
  t.gB = tile == ntiles - 1 ? G : min(ptr_lower_bound(ptr, G + 1, n1), G);
  if (t.gB < t.gA) t.gB = t.gA;
  t.has_chunk = 0;
  if (t.gA > 0) {
    const int g = t.gA - 1;
    const int gbeg = min(ptr[g], V), gend = min(ptr[g + 1], V);
    if (gbeg < n0 && gend > n0 && gend - gbeg > kChunk) {
      const int k = (n0 - gbeg + kChunk - 1) / kChunk;
      const int s = gbeg + k * kChunk;
      if (s < gend && s < n1) {
        t.has_chunk = 1;
        t.chunk.g = g;
        t.chunk.gbeg = gbeg;
        t.chunk.gend = gend;
        t.chunk.beg = s;
        t.chunk.end = min(s + kChunk, gend);
        t.chunk.slot = 0;
      }
    }
  }
  return t;
}

// the workspace slot of chunk k of a graph beginning at node gbeg
__device__ __forceinline__ int64_t pool_slot_of(int gbeg, int k) {
  return (int64_t)((gbeg + k * kChunk) / kChunk) * 2 + (k == 0 ? 1 : 0);
}

// dst[h] = reduction over the nodes v of [beg, end) of f(v, h), for every head, by one wave (dst: LDS of the wave).
// heads a power of two <= 64: the lanes run over the (node, head) pairs and a lane stays on one head; otherwise head by head.
template <bool MAX, class F>
__device__ __forceinline__ void wave_head_reduce(int heads, int beg, int end, float* dst, F f) {
  const int lane = threadIdx.x & 63;
  const float init = MAX ? kFloatLowest : 0.f;
  if (heads <= 64 && (heads & (heads - 1)) == 0) {
    const int sh = __ffs(heads) - 1;
    const int h = lane & (heads - 1);
    const int n = (end - beg) << sh;
    float a = init;
    for (int i = lane; i < n; i += 64) {
      const float x = f(beg + (i >> sh), h);
      a = MAX ? fmaxf(a, x) : a + x;
    }
    for (int d = heads; d < 64; d <<= 1) {
      const float o = __shfl_xor(a, d, 64);
      a = MAX ? fmaxf(a, o) : a + o;
    }
    if (lane < heads) dst[h] = a;
  } else {
    for (int h = 0; h < heads; ++h) {
      float a = init;
      for (int v = beg + lane; v < end; v += 64) {
        const float x = f(v, h);
        a = MAX ? fmaxf(a, x) : a + x;
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_xor(a, d, 64);
        a = MAX ? fmaxf(a, o) : a + o;
      }
      if (lane == 0) dst[h] = a;
    }
  }
  wave_sync();
}

template <int VEC>
struct Row {
  float x[VEC];
};
template <int VEC>
__device__ __forceinline__ Row<VEC> row_load(const float* p) {
  Row<VEC> r;
  if (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    r.x[0] = v.x; r.x[1 % VEC] = v.y; r.x[2 % VEC] = v.z; r.x[3 % VEC] = v.w;
  } else {
    r.x[0] = *p;
  }
  return r;
}
template <int VEC>
__device__ __forceinline__ void row_store(float* p, const Row<VEC>& r) {
  if (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(r.x[0], r.x[1 % VEC], r.x[2 % VEC], r.x[3 % VEC]);
  else *p = r.x[0];
}

struct PoolShape {
  int V, G, GD, heads, kind;
  int cl_shift;  // log2 of the lanes along the features (CL); 64 / CL lanes along the nodes
  int ntiles;
  int64_t ws_stride;  // floats per workspace slot
  float lo, hi;
};

// ---- forward ----------------------------------------------------------------------------------------------------------
// slot layout (floats): [0, GD) weighted sums; SOFTMAX: [GD, GD + heads) running max, [GD + heads, GD + 2 heads) sum of exp
template <int VEC>
__global__ void __launch_bounds__(256)
pool_forward_kernel(PoolShape p, const int32_t* __restrict__ ptr, const float* __restrict__ T, int64_t ldT,
                    const float* __restrict__ S, int64_t ldS, float* __restrict__ out, float* __restrict__ w, int64_t ldw,
                    float* __restrict__ ws) {
  extern __shared__ float pool_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* stat_m = pool_lds + (size_t)wave * 2 * p.heads;  // per head: max, then 1 / (sum + 1e-7) (1 for a chunk)
  float* stat_i = stat_m + p.heads;
  const int CL = 1 << p.cl_shift, NL = 64 >> p.cl_shift;
  const int cl = lane & (CL - 1), nl = lane >> p.cl_shift;
  const int CB = CL * VEC;
  const int ph = p.GD / p.heads;
  const float lo = p.lo, hi = p.hi;
  const PoolTile tile = pool_tile(ptr, p.V, p.G, blockIdx.x, p.ntiles);
  const int nseg = tile.num_segments();
  for (int si = wave; si < nseg; si += 4) {
    const PoolSeg s = tile.segment(si);
    float* slot = s.slot >= 0 ? ws + ((int64_t)blockIdx.x * 2 + s.slot) * p.ws_stride : nullptr;
    if (p.kind == TFGNN_POOL_SOFTMAX) {
      wave_head_reduce<true>(p.heads, s.beg, s.end, stat_m, [&](int v, int h) { return S[(int64_t)v * ldS + h]; });
      wave_head_reduce<false>(p.heads, s.beg, s.end, stat_i,
                              [&](int v, int h) { return expf(S[(int64_t)v * ldS + h] - stat_m[h]); });
      if (slot) {
        for (int h = lane; h < p.heads; h += 64) {
          slot[p.GD + h] = stat_m[h];
          slot[p.GD + p.heads + h] = stat_i[h];
        }
        wave_sync();
        for (int h = lane; h < p.heads; h += 64) stat_i[h] = 1.f;
      } else {
        for (int h = lane; h < p.heads; h += 64) stat_i[h] = 1.f / (stat_i[h] + kSmallNumber);
      }
      wave_sync();
      if (!slot) {
        const int n = (s.end - s.beg) * p.heads;
        for (int i = lane; i < n; i += 64) {
          const int v = s.beg + i / p.heads, h = i % p.heads;
          w[(int64_t)v * ldw + h] = expf(S[(int64_t)v * ldS + h] - stat_m[h]) * stat_i[h];
        }
      }
    }
    for (int c0 = 0; c0 < p.GD; c0 += CB) {
      const int c = c0 + cl * VEC;
      const bool active = c < p.GD;
      int hj[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) hj[j] = active ? (c + j) / ph : 0;
      float acc[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
      if (active) {
#pragma unroll 4
        for (int v = s.beg + nl; v < s.end; v += NL) {
          const Row<VEC> x = row_load<VEC>(T + (int64_t)v * ldT + c);
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            float wt = 1.f;
            if (p.kind == TFGNN_POOL_SIGMOID) wt = S[(int64_t)v * ldS + hj[j]];
            else if (p.kind == TFGNN_POOL_SOFTMAX) wt = expf(S[(int64_t)v * ldS + hj[j]] - stat_m[hj[j]]) * stat_i[hj[j]];
            acc[j] += wt * clip_value(x.x[j], lo, hi);
          }
        }
      }
      for (int d = CL; d < 64; d <<= 1) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] += __shfl_xor(acc[j], d, 64);
      }
      if (active && nl == 0) {
        Row<VEC> r;
        const int cnt = s.gend - s.gbeg;
#pragma unroll
        for (int j = 0; j < VEC; ++j) r.x[j] = (!slot && p.kind == TFGNN_POOL_AVERAGE) ? acc[j] / (float)(cnt > 0 ? cnt : 1) : acc[j];
        row_store<VEC>(slot ? slot + c : out + (int64_t)s.g * p.GD + c, r);
      }
    }
    wave_sync();  // the next segment rewrites the wave's statistics
  }
}

// second launch: the graphs of more than kChunk nodes.  Every tile that owns a chunk combines the statistics of all chunks of
// that graph in ascending order (SOFTMAX) and writes the weights of its own nodes; the tile of chunk 0 also combines the sums.
__global__ void __launch_bounds__(256)
pool_forward_combine_kernel(PoolShape p, const int32_t* __restrict__ ptr, const float* __restrict__ S, int64_t ldS,
                            float* __restrict__ out, float* __restrict__ w, int64_t ldw, const float* __restrict__ ws) {
  extern __shared__ float pool_lds[];
  __shared__ float red[256];
  float* stat_m = pool_lds;
  float* stat_i = pool_lds + p.heads;
  const int tid = threadIdx.x;
  const PoolTile tile = pool_tile(ptr, p.V, p.G, blockIdx.x, p.ntiles);
  const int ph = p.GD / p.heads;
  for (int which = 0; which < 2; ++which) {  // uniform over the workgroup
    PoolSeg s;
    if (which == 0) {
      if (!tile.has_chunk) continue;
      s = tile.chunk;
    } else {
      if (tile.gB <= tile.gA) continue;
      s = tile.segment(tile.has_chunk + (tile.gB - tile.gA) - 1);
      if (s.slot < 0) continue;
    }
    const int K = (s.gend - s.gbeg + kChunk - 1) / kChunk;
    const bool first = s.beg == s.gbeg;
    if (p.kind == TFGNN_POOL_SOFTMAX) {
      for (int h = tid; h < p.heads; h += 256) {
        float m = kFloatLowest;
        for (int k = 0; k < K; ++k) m = fmaxf(m, ws[pool_slot_of(s.gbeg, k) * p.ws_stride + p.GD + h]);
        float sum = 0.f;
        for (int k = 0; k < K; ++k) {
          const float* slot = ws + pool_slot_of(s.gbeg, k) * p.ws_stride + p.GD;
          sum += slot[p.heads + h] * expf(slot[h] - m);
        }
        stat_m[h] = m;
        stat_i[h] = 1.f / (sum + kSmallNumber);
      }
      __syncthreads();
      const int n = (s.end - s.beg) * p.heads;
      for (int i = tid; i < n; i += 256) {
        const int v = s.beg + i / p.heads, h = i % p.heads;
        w[(int64_t)v * ldw + h] = expf(S[(int64_t)v * ldS + h] - stat_m[h]) * stat_i[h];
      }
    }
    if (first) {
      // columns over CW lanes, the chunks over 256 / CW groups of them; the groups' sums are added in ascending order
      int CW = 1;
      while (CW < p.GD && CW < 256) CW <<= 1;
      const int KG = 256 / CW, cw = tid % CW, kg = tid / CW;
      const int cnt = s.gend - s.gbeg;
      for (int c0 = 0; c0 < p.GD; c0 += CW) {
        const int c = c0 + cw;
        float acc = 0.f;
        if (c < p.GD) {
          const int h = c / ph;
#pragma unroll 4
          for (int k = kg; k < K; k += KG) {
            const float* slot = ws + pool_slot_of(s.gbeg, k) * p.ws_stride;
            float x = slot[c];
            if (p.kind == TFGNN_POOL_SOFTMAX) x *= expf(slot[p.GD + h] - stat_m[h]);
            acc += x;
          }
        }
        red[tid] = acc;
        __syncthreads();
        if (kg == 0 && c < p.GD) {
          float t = red[cw];
          for (int q = 1; q < KG; ++q) t += red[q * CW + cw];
          if (p.kind == TFGNN_POOL_SOFTMAX) t *= stat_i[c / ph];
          if (p.kind == TFGNN_POOL_AVERAGE) t /= (float)(cnt > 0 ? cnt : 1);
          out[(int64_t)s.g * p.GD + c] = t;
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// slot layout (floats): SOFTMAX [0, heads) sum over the chunk of w * dw
template <int VEC>
__global__ void __launch_bounds__(256)
pool_backward_kernel(PoolShape p, const int32_t* __restrict__ ptr, const float* __restrict__ dOut, const float* __restrict__ T,
                     int64_t ldT, const float* __restrict__ w, int64_t ldw, float* __restrict__ dT, int64_t lddT,
                     float* dS, int64_t lddS, float* __restrict__ ws) {
  extern __shared__ float pool_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int CL = 1 << p.cl_shift, NL = 64 >> p.cl_shift;
  const int cl = lane & (CL - 1), nl = lane >> p.cl_shift;
  const int CB = CL * VEC;
  const int ph = p.GD / p.heads;
  float* stat_t = pool_lds + (size_t)wave * (p.heads + (size_t)NL * p.GD);  // per head: sum of w * dw
  float* prod = stat_t + p.heads;                                           // [NL, GD]: clip(T) * dOut of the nodes in flight
  const float lo = p.lo, hi = p.hi;
  const bool weighted = p.kind == TFGNN_POOL_SOFTMAX || p.kind == TFGNN_POOL_SIGMOID;
  const bool need_dw = weighted && dS != nullptr;
  const PoolTile tile = pool_tile(ptr, p.V, p.G, blockIdx.x, p.ntiles);
  const int nseg = tile.num_segments();
  for (int si = wave; si < nseg; si += 4) {
    const PoolSeg s = tile.segment(si);
    const float* dg = dOut + (int64_t)s.g * p.GD;
    const int cnt = s.gend - s.gbeg;
    const float wconst = p.kind == TFGNN_POOL_AVERAGE ? 1.f / (float)(cnt > 0 ? cnt : 1) : 1.f;
    for (int v0 = s.beg; v0 < s.end; v0 += NL) {
      const int v = v0 + nl;
      if (v < s.end) {
        for (int c0 = 0; c0 < p.GD; c0 += CB) {
          const int c = c0 + cl * VEC;
          if (c >= p.GD) continue;
          const Row<VEC> x = row_load<VEC>(T + (int64_t)v * ldT + c);
          const Row<VEC> d = row_load<VEC>(dg + c);
          Row<VEC> r;
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const float wt = weighted ? w[(int64_t)v * ldw + (c + j) / ph] : wconst;
            const float xv = x.x[j];
            r.x[j] = (xv >= lo && xv <= hi) ? wt * d.x[j] : 0.f;  // tfgnn_clip_backward's mask
            if (need_dw) prod[nl * p.GD + c + j] = clip_value(xv, lo, hi) * d.x[j];
          }
          row_store<VEC>(dT + (int64_t)v * lddT + c, r);
        }
      }
      if (need_dw) {
        wave_sync();
        const int n = min(NL, s.end - v0) * p.heads;
        for (int i = lane; i < n; i += 64) {
          const int r = i / p.heads, h = i % p.heads;
          const float* pr = prod + r * p.GD + h * ph;
          float a = 0.f;
          for (int j = 0; j < ph; ++j) a += pr[j];
          dS[(int64_t)(v0 + r) * lddS + h] = a;  // SIGMOID: final.  SOFTMAX: dw, replaced below / by the second launch
        }
        wave_sync();
      }
    }
    if (need_dw && p.kind == TFGNN_POOL_SOFTMAX) {
      __threadfence_block();  // this wave's dw, read back by other lanes of it
      wave_head_reduce<false>(p.heads, s.beg, s.end, stat_t,
                              [&](int v, int h) { return w[(int64_t)v * ldw + h] * dS[(int64_t)v * lddS + h]; });
      if (s.slot >= 0) {
        float* slot = ws + ((int64_t)blockIdx.x * 2 + s.slot) * p.ws_stride;
        for (int h = lane; h < p.heads; h += 64) slot[h] = stat_t[h];
      } else {
        const int n = (s.end - s.beg) * p.heads;
        for (int i = lane; i < n; i += 64) {
          const int v = s.beg + i / p.heads, h = i % p.heads;
          const int64_t at = (int64_t)v * lddS + h;
          dS[at] = w[(int64_t)v * ldw + h] * (dS[at] - stat_t[h]);
        }
      }
      wave_sync();
    }
  }
}

// second launch (SOFTMAX with dS): the chunks of graphs of more than kChunk nodes: t = sum of the chunks' sums in ascending
// order, dS = w * (dw - t) over the tile's own chunk
__global__ void __launch_bounds__(256)
pool_backward_combine_kernel(PoolShape p, const int32_t* __restrict__ ptr, const float* __restrict__ w, int64_t ldw, float* dS,
                             int64_t lddS, const float* __restrict__ ws) {
  extern __shared__ float pool_lds[];
  const int tid = threadIdx.x;
  const PoolTile tile = pool_tile(ptr, p.V, p.G, blockIdx.x, p.ntiles);
  for (int which = 0; which < 2; ++which) {
    PoolSeg s;
    if (which == 0) {
      if (!tile.has_chunk) continue;
      s = tile.chunk;
    } else {
      if (tile.gB <= tile.gA) continue;
      s = tile.segment(tile.has_chunk + (tile.gB - tile.gA) - 1);
      if (s.slot < 0) continue;
    }
    const int K = (s.gend - s.gbeg + kChunk - 1) / kChunk;
    for (int h = tid; h < p.heads; h += 256) {
      float t = 0.f;
      for (int k = 0; k < K; ++k) t += ws[pool_slot_of(s.gbeg, k) * p.ws_stride + h];
      pool_lds[h] = t;
    }
    __syncthreads();
    const int n = (s.end - s.beg) * p.heads;
    for (int i = tid; i < n; i += 256) {
      const int v = s.beg + i / p.heads, h = i % p.heads;
      const int64_t at = (int64_t)v * lddS + h;
      dS[at] = w[(int64_t)v * ldw + h] * (dS[at] - pool_lds[h]);
    }
    __syncthreads();
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
static int64_t pool_ws_stride(int GD, int heads, int kind) { return (int64_t)GD + (kind == TFGNN_POOL_SOFTMAX ? 2 * (int64_t)heads : 0); }

static size_t pool_workspace_bytes(int64_t V, int GD, int heads, int kind) {
  if (V <= kChunk || GD <= 0 || heads <= 0) return 0;  // no graph can have more than kChunk nodes: nothing to combine
  return (size_t)(ceil_div(V, kChunk) * 2 * pool_ws_stride(GD, heads, kind)) * sizeof(float);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static PoolShape pool_shape(int64_t V, int64_t G, int GD, int heads, int kind, float lo, float hi, int vec) {
  PoolShape p;
  p.V = (int)V; p.G = (int)G; p.GD = GD; p.heads = heads; p.kind = kind;
  p.lo = lo; p.hi = hi;
  p.ntiles = (int)ceil_div(V, kChunk);
  p.ws_stride = pool_ws_stride(GD, heads, kind);
  int sh = 0;
  while ((1 << sh) * vec < GD && sh < 6) ++sh;
  p.cl_shift = sh;
  return p;
}

// checks shared by the two calls, in the order the header promises: everything that needs no pointer first
#define TFGNN_POOL_CHECK_SIZES(name, a)                                                                                       \
  TFGNN_REQUIRE((a)->kind >= TFGNN_POOL_SOFTMAX && (a)->kind <= TFGNN_POOL_AVERAGE, name ": unknown weighting kind %d", (a)->kind); \
  TFGNN_REQUIRE((a)->V >= 0 && (a)->G >= 0 && (a)->GD >= 0, name ": negative size");                                         \
  TFGNN_REQUIRE((a)->V < ((int64_t)1 << 31) - kChunk && (a)->G < ((int64_t)1 << 31) - 1, name ": too large");                 \
  TFGNN_REQUIRE((a)->heads > 0 && (a)->GD % (a)->heads == 0, name ": heads (%d) must divide the width (%d)", (a)->heads, (a)->GD); \
  TFGNN_REQUIRE((a)->lo <= (a)->hi, name ": lower bound above upper bound (or NaN)");                                         \
  if ((a)->V == 0 || (a)->G == 0 || (a)->GD == 0) return TFGNN_OK;                                                            \
  TFGNN_REQUIRE((a)->workspace_bytes >= pool_workspace_bytes((a)->V, (a)->GD, (a)->heads, (a)->kind) &&                       \
                    ((a)->workspace || pool_workspace_bytes((a)->V, (a)->GD, (a)->heads, (a)->kind) == 0),                    \
                name ": workspace of %zu bytes, tfgnn_pool_workspace_bytes asks for %zu", (a)->workspace_bytes,               \
                pool_workspace_bytes((a)->V, (a)->GD, (a)->heads, (a)->kind))

}  // namespace tfgnn

using namespace tfgnn;

extern "C" size_t tfgnn_pool_workspace_bytes(int64_t V, int64_t G, int GD, int heads, int kind) {
  if (G <= 0) return 0;
  return pool_workspace_bytes(V, GD, heads, kind);
}

extern "C" int tfgnn_pool_launch_counts(int64_t* out_counts, int n) {
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_pool_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i < 2 ? g_pool_launches[i].load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

extern "C" int tfgnn_pool_forward(const tfgnn_pool_forward_args* a, void* stream) {
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_pool_forward_args),
                "tfgnn_pool_forward: args is NULL or was built against another header (struct_size)");
  TFGNN_POOL_CHECK_SIZES("tfgnn_pool_forward", a);
  const bool scored = a->kind == TFGNN_POOL_SOFTMAX || a->kind == TFGNN_POOL_SIGMOID;
  TFGNN_REQUIRE(a->ptr && a->T && a->out && (!scored || a->S) && (a->kind != TFGNN_POOL_SOFTMAX || a->w),
                "tfgnn_pool_forward: NULL pointer");
  TFGNN_REQUIRE(a->ldT >= a->GD && (!scored || a->ldS >= a->heads) && (a->kind != TFGNN_POOL_SOFTMAX || a->ldw >= a->heads),
                "tfgnn_pool_forward: leading dimension smaller than the row");
  if (a->GD > kPoolMaxWidth) {
    set_error("tfgnn_pool_forward: rows of more than %d floats are not supported", kPoolMaxWidth);
    return TFGNN_ERR_UNSUPPORTED;
  }
  const int vec = (a->GD % 4 == 0 && a->ldT % 4 == 0 && aligned16(a->T) && aligned16(a->out) && aligned16(a->workspace) &&
                   pool_ws_stride(a->GD, a->heads, a->kind) % 4 == 0) ? 4 : 1;
  const PoolShape p = pool_shape(a->V, a->G, a->GD, a->heads, a->kind, a->lo, a->hi, vec);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)4 * 2 * a->heads * sizeof(float);
  float* ws = (float*)a->workspace;
  if (vec == 4)
    hipLaunchKernelGGL(pool_forward_kernel<4>, dim3(p.ntiles), dim3(256), lds, s, p, a->ptr, a->T, a->ldT, a->S, a->ldS, a->out, a->w,
                       a->ldw, ws);
  else
    hipLaunchKernelGGL(pool_forward_kernel<1>, dim3(p.ntiles), dim3(256), lds, s, p, a->ptr, a->T, a->ldT, a->S, a->ldS, a->out, a->w,
                       a->ldw, ws);
  TFGNN_LAUNCH_CHECK();
  g_pool_launches[0].fetch_add(1, std::memory_order_relaxed);
  if (a->V > kChunk) {  // only then can a graph have been cut into chunks
    hipLaunchKernelGGL(pool_forward_combine_kernel, dim3(p.ntiles), dim3(256), (size_t)2 * a->heads * sizeof(float), s, p, a->ptr,
                       a->S, a->ldS, a->out, a->w, a->ldw, ws);
    TFGNN_LAUNCH_CHECK();
    g_pool_launches[0].fetch_add(1, std::memory_order_relaxed);
  }
  return TFGNN_OK;
}

extern "C" int tfgnn_pool_backward(const tfgnn_pool_backward_args* a, void* stream) {
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_pool_backward_args),
                "tfgnn_pool_backward: args is NULL or was built against another header (struct_size)");
  TFGNN_POOL_CHECK_SIZES("tfgnn_pool_backward", a);
  const bool scored = a->kind == TFGNN_POOL_SOFTMAX || a->kind == TFGNN_POOL_SIGMOID;
  TFGNN_REQUIRE(a->ptr && a->dOut && a->T && a->dT && (!scored || a->w), "tfgnn_pool_backward: NULL pointer");
  TFGNN_REQUIRE(scored || !a->dS, "tfgnn_pool_backward: dS must be NULL for the kinds without scores");
  TFGNN_REQUIRE(a->ldT >= a->GD && a->lddT >= a->GD && (!scored || a->ldw >= a->heads) && (!a->dS || a->lddS >= a->heads),
                "tfgnn_pool_backward: leading dimension smaller than the row");
  if (a->GD > kPoolMaxWidth) {
    set_error("tfgnn_pool_backward: rows of more than %d floats are not supported", kPoolMaxWidth);
    return TFGNN_ERR_UNSUPPORTED;
  }
  const int vec = (a->GD % 4 == 0 && a->ldT % 4 == 0 && a->lddT % 4 == 0 && aligned16(a->T) && aligned16(a->dT) && aligned16(a->dOut)) ? 4 : 1;
  const PoolShape p = pool_shape(a->V, a->G, a->GD, a->heads, a->kind, a->lo, a->hi, vec);
  hipStream_t s = (hipStream_t)stream;
  const int NL = 64 >> p.cl_shift;
  const size_t lds = (size_t)4 * (a->heads + (size_t)NL * a->GD) * sizeof(float);
  float* ws = (float*)a->workspace;
  if (vec == 4)
    hipLaunchKernelGGL(pool_backward_kernel<4>, dim3(p.ntiles), dim3(256), lds, s, p, a->ptr, a->dOut, a->T, a->ldT, a->w, a->ldw, a->dT,
                       a->lddT, a->dS, a->lddS, ws);
  else
    hipLaunchKernelGGL(pool_backward_kernel<1>, dim3(p.ntiles), dim3(256), lds, s, p, a->ptr, a->dOut, a->T, a->ldT, a->w, a->ldw, a->dT,
                       a->lddT, a->dS, a->lddS, ws);
  TFGNN_LAUNCH_CHECK();
  g_pool_launches[1].fetch_add(1, std::memory_order_relaxed);
  if (a->kind == TFGNN_POOL_SOFTMAX && a->dS && a->V > kChunk) {
    hipLaunchKernelGGL(pool_backward_combine_kernel, dim3(p.ntiles), dim3(256), (size_t)a->heads * sizeof(float), s, p, a->ptr, a->w,
                       a->ldw, a->dS, a->lddS, ws);
    TFGNN_LAUNCH_CHECK();
    g_pool_launches[1].fetch_add(1, std::memory_order_relaxed);
  }
  return TFGNN_OK;
}
