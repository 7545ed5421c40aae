// Gather + segment reduce over a CSR: the bandwidth-bound half of the message-passing hot path.
//
//   out[r, :] = post_act( row_scale[r] * REDUCE_{e in row r} pre_act( w_e * in[col[e], :] ) )
//
// One call replaces, for one edge-bucketed view of the graph,
//   tf.nn.embedding_lookup(node_embeddings, edge_sources)          message_passing.py:197-199
//   the per-message 1/(c + 1e-7) scaling                             gnn_edge_mlp.py:102-106
//   tf.concat over edge types                                        message_passing.py:166-167
//   tf.math.unsorted_segment_{sum,max,mean,sqrt_n}                   utils/param_helpers.py:9-14
//   (RGAT) attention-weighted per-head unsorted_segment_sum          rgat.py:154-160
// without ever materialising the [E, D] gathered tensor (1.15 GB per layer at cfg-2).
//
// Work decomposition (wave64): a wave is split into 64/LPR groups of LPR lanes; a group owns one
// CSR row and a window of LPR*VPL float4 chunks of the feature dimension.  Lane j of the group
// owns chunks j, j+LPR, ... so that each load instruction of a group reads LPR*16 contiguous bytes
// of one source row (>= one 128 B line for LPR >= 8).  Edges are walked UNROLL at a time to keep
// UNROLL*VPL 16-byte loads in flight per lane; their column indices and weights are read LPR edges
// at a time, one edge per lane, and handed round inside the group (EdgeBlocks).  Accumulation order inside a row is the CSR order
// (cols ascending) -> bit-reproducible, no atomics.
//
// Skew (R-MAT hubs): with a plan (graph views), rows longer than LONG_ROW_THRESHOLD are skipped by
// the row kernel and cut into items of ITEM_CHUNK edges; one workgroup per item, its groups each
// take a contiguous slice of the item, partial sums are combined through LDS in group order.  Rows
// made of several items go through a scratch buffer: every item workgroup stores its partial row
// (write-through), then counts its arrival on the row's counter in the graph handle; the workgroup that
// arrives last adds the row's partial rows in item order and writes the result (finish_multi_row) - no second
// launch, nobody waits, and the order of the sum does not depend on who arrives last.
// Everything stays deterministic.
//
// blockIdx.y walks feature windows.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "common.hpp"
#include "graph.hpp"
#include "sp16.hpp"

namespace tfgnn {

template <int VEC>
struct VecT;
template <>
struct VecT<4> {
  using type = float4;
};
template <>
struct VecT<1> {
  using type = float;
};

template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type vload(const float* p);
template <>
__device__ __forceinline__ float4 vload<4>(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
template <>
__device__ __forceinline__ float vload<1>(const float* p) {
  return *p;
}

template <int VEC>
__device__ __forceinline__ void vstore(float* p, const float* v);
template <>
__device__ __forceinline__ void vstore<4>(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <>
__device__ __forceinline__ void vstore<1>(float* p, const float* v) {
  *p = v[0];
}

template <int VEC>
__device__ __forceinline__ void vunpack(const typename VecT<VEC>::type& v, float* o);
template <>
__device__ __forceinline__ void vunpack<4>(const float4& v, float* o) {
  o[0] = v.x;
  o[1] = v.y;
  o[2] = v.z;
  o[3] = v.w;
}
template <>
__device__ __forceinline__ void vunpack<1>(const float& v, float* o) {
  o[0] = v;
}

// MODE 0: sum, optional scalar edge weight          (RGCN / GGNN / RGIN forward and backward)
// MODE 1: sum, per-head edge weights ew[e, K]       (RGAT)
// MODE 2: general: runtime max / pre-activation, optional scalar edge weight
// MODE 3: MODE 1 + per edge and head the inner product of the gathered row with a row that belongs to the CSR row
//         (RGAT backward: d attention[e, k] = <Y[(src_e, l_e)], d_agg[tgt_e]>_k rides on the by-source gather that reads
//         d_agg[tgt_e] anyway - round 4; before, rgat_edge_dot read Y[(src_e, l_e)] per edge in a pass of its own)
enum { MODE_SUM = 0, MODE_HEADS = 1, MODE_GENERAL = 2, MODE_HEADS_DOT = 3 };
__host__ __device__ constexpr bool mode_heads(int mode) { return mode == MODE_HEADS || mode == MODE_HEADS_DOT; }

// value of the lane at distance 1 << S inside its aligned group of 2 << S lanes (S = 3, 2: the mirrored lane - same thing for a sum)
template <int S>
__device__ __forceinline__ float dpp_partner(float v) {
  constexpr int ctrl = S == 0 ? 0xB1 : S == 1 ? 0x4E : S == 2 ? 0x141 : 0x140;  // quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false));
}
// N values per lane, each to be summed over the 1 << L2 consecutive lanes of the lane's group (N <= 1 << L2): instead of N
// butterflies the lanes split the values among themselves - at the top log2(N) distances a lane keeps the half of its values
// its lane bit selects and receives the partner's partial sums of that half - then one butterfly finishes the value left.
// -> the complete sum of value number `which` (lanes that differ only in the bits below the splitting ones hold copies)
template <int N, int L2>
__device__ __forceinline__ float dpp_split_sum(const float (&p)[N], int lane, int& which) {
  static_assert(N == 1 || N == 2 || N == 4, "values per lane");
  static_assert((1 << L2) >= N && L2 <= 4, "group");
  if constexpr (N == 4) {
    const bool hi = (lane >> (L2 - 1)) & 1;
    float q[2];
    q[0] = (hi ? p[2] : p[0]) + dpp_partner<L2 - 1>(hi ? p[0] : p[2]);
    q[1] = (hi ? p[3] : p[1]) + dpp_partner<L2 - 1>(hi ? p[1] : p[3]);
    int w;
    const float r = dpp_split_sum<2, L2 - 1>(q, lane, w);
    which = (hi ? 2 : 0) + w;
    return r;
  } else if constexpr (N == 2) {
    const bool hi = (lane >> (L2 - 1)) & 1;
    float q[1];
    q[0] = (hi ? p[1] : p[0]) + dpp_partner<L2 - 1>(hi ? p[0] : p[1]);
    int w;
    const float r = dpp_split_sum<1, L2 - 1>(q, lane, w);
    which = hi ? 1 : 0;
    return r;
  } else {
    float v = p[0];
    if constexpr (L2 >= 4) v += dpp_partner<3>(v);
    if constexpr (L2 >= 3) v += dpp_partner<2>(v);
    if constexpr (L2 >= 2) v += dpp_partner<1>(v);
    if constexpr (L2 >= 1) v += dpp_partner<0>(v);
    which = 0;
    return v;
  }
}

// sum over the 1 << log2n (<= 16) consecutive lanes a lane belongs to (DPP: no LDS traffic); every lane gets the sum
__device__ __forceinline__ float dpp_group_sum(float v, int log2n) {
  int x;
  if (log2n >= 1) { x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false); v += __int_as_float(x); }   // quad_perm [1,0,3,2]
  if (log2n >= 2) { x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false); v += __int_as_float(x); }   // quad_perm [2,3,0,1]
  if (log2n >= 3) { x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false); v += __int_as_float(x); }  // row_half_mirror
  if (log2n >= 4) { x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false); v += __int_as_float(x); }  // row_mirror
  return v;
}

struct GatherArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* short_rows;  // nullable: the rows the row workgroups handle, longest first (CsrPlan)
  int64_t num_short;
  const float* ew;         // nullable; [E] or [E, ew_heads]
  const float* row_scale;  // nullable
  int64_t num_rows;
  const float* in;
  int64_t ld_in;
  int width;  // floats
  float* out;
  int64_t ld_out;
  int pre_act;
  int post_act;
  int is_max;
  int ew_heads;    // K (MODE_HEADS)
  int head_width;  // floats per head (MODE_HEADS)
  // MODE_HEADS_DOT: dot_out[pos(e) * ew_heads + k] = sum over head k of in[col[e]] * dot_rows[CSR row of e]; pos = dot_pos[e]
  // (nullable: e).  head_width / 4 = 1 << dot_lph_log2 lanes hold a head (<= lanes per row, <= 16)
  const float* dot_rows;
  int64_t ld_dot;
  float* dot_out;
  const int32_t* dot_pos;
  int dot_lph_log2;
  int long_threshold;  // rows longer than this are left to the item kernels (0 = never)
  const int32_t* out_row_map;  // nullable: output row of CSR row r is out_row_map[r]; < 0 = no output
  // item pass
  const int32_t* item_row;
  const int32_t* item_chunk;
  const int32_t* item_slot;
  const int32_t* item_multi;
  float* partial;  // [num_partials, width]
  int item_chunk_edges;
  // rows made of several items: combined by their last-arriving item workgroup
  const int32_t* multi_base;
  const int32_t* multi_n;
  uint32_t* arrive;  // [num_multi][ARRIVE_WINDOWS], zero between launches
  // SP16 output (kernels instantiated with SP = true; MODE_SUM, float4 path, one feature window): the row sums are
  // written as the split fp16 operand of the f16x2 products (csrc/gemm_sp.hip) instead of fp32
  uint8_t* out_sp;         // [rows] x ld_out_sp bytes
  int64_t ld_out_sp;
  float* inv_out;          // [rows] 2^-e of every output row (not written when fixed_inv is given)
  const float* fixed_inv;  // nullable: one caller-chosen 2^-e for the whole tensor
  bool multi_pairs;  // host only: the short rows go two to a lane group, one edge of each per round (gather_rows_block_multi)
  // > 0: short_rows[0, rider_ne) are the non-empty short rows and the only ones with a lane group of their own; the group
  // of slot i also zero-fills the empty rows short_rows[i + rider_ne], [i + 2 * rider_ne], .. (< num_short) while its first
  // source rows are in flight (empty_riders).  0: every short row has its own group
  int64_t rider_ne;
};

// scale of one output row from the maximum (sp_absmax_bits) over its LANES lanes (lanes of one group are contiguous)
template <int LANES>
__device__ __forceinline__ float sp_row_scale(const GatherArgs& a, unsigned mx, int64_t orow, bool writer) {
  float iv, sc;
  if (a.fixed_inv) {
    iv = a.fixed_inv[0];
    sc = 1.f / iv;
  } else {
#pragma unroll
    for (int o = LANES / 2; o; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, LANES));
    sc = sp_scale_for_max(__uint_as_float(mx), &iv);
    if (writer) a.inv_out[orow] = iv;
  }
  return sc;
}

// ---- the edge walk's index blocks (round 12) --------------------------------------------------------------------------------
// A lane group reads what it needs to know about its edges - column index, scalar weight, (MODE_HEADS_DOT) output position -
// LPR consecutive edges at a time: lane j of the group loads edge p0 + j of the block, one coalesced load per array.  An
// edge's values reach all lanes of the group by a cross-lane read (__shfl inside the group: ds_bpermute, no memory access).
// Before, every lane of the group loaded the same col[e] at the top of every round and waited for it with no source row in
// flight: two latencies in series per round; now the walk waits for indices once per LPR edges (a typed short row of <= 48
// edges: at most three times).  Keeping the block after the current one in flight as well was measured and dropped: the two
// registers it holds across the loop took the SP16 kernel at width 320 from 90 to 107 registers, 5 waves per SIMD to 4, and
// the launch from 84 to 86 us (NOTEBOOK section 46).
// All lanes of a group walk the same edges, so the cross-lane reads are convergent inside the group; other groups of the
// wave may be anywhere, their lanes are not read.
template <int MODE>
struct EdgeBlock {
  int32_t idx;  // lanes past the end of the walk: 0 (never used for a load)
  float w;
  int32_t pos;
};
template <int MODE>
__device__ __forceinline__ EdgeBlock<MODE> load_edge_block(const GatherArgs& a, int32_t p, int32_t end) {
  EdgeBlock<MODE> b;
  b.idx = 0;
  b.w = 1.f;
  b.pos = p;
  if (p < end) {
    b.idx = a.col[p];
    if (!mode_heads(MODE) && a.ew) b.w = a.ew[p];
    if (MODE == MODE_HEADS_DOT && a.dot_pos) b.pos = a.dot_pos[p];
  }
  return b;
}
// the block being walked (first edge `base`)
template <int LPR, int MODE>
struct EdgeBlocks {
  EdgeBlock<MODE> cur;
  int32_t base, end;
  int gl;
  __device__ __forceinline__ void start(const GatherArgs& a, int32_t beg, int32_t end_) {
    gl = threadIdx.x % LPR;
    base = beg;
    end = end_;
    cur = load_edge_block<MODE>(a, beg + gl, end);
  }
  // make the block that holds edge e (>= base, at most one block on) the current one
  __device__ __forceinline__ void seek(const GatherArgs& a, int32_t e) {
    if (e - base >= LPR) {
      base += LPR;
      cur = load_edge_block<MODE>(a, base + gl, end);
    }
  }
  __device__ __forceinline__ int32_t idx(int32_t e) const { return __shfl(cur.idx, e - base, LPR); }
  __device__ __forceinline__ float w(int32_t e) const { return __shfl(cur.w, e - base, LPR); }
  __device__ __forceinline__ int32_t pos(int32_t e) const { return __shfl(cur.pos, e - base, LPR); }
};

// Which walks read their indices in blocks: the ones with rounds of two edges (rows of 256 floats and more, where a round
// is short and a row has many of them), except MODE_GENERAL.  The variants with rounds of four and eight edges keep one index
// load per edge and round: their wait is spread over a longer round, the (node, type) buckets of a molecule batch hold fewer
// edges than one round, and with the blocks qm9-ggnn (width 128) ran 0.26 % slower in three pairs of three.  MODE_GENERAL:
// the block registers cost its narrow variants a wave per SIMD (80 -> 86, 77 -> 84 registers; tools/kernel_resources.py).
__host__ __device__ constexpr bool index_blocks(int mode, int unroll) { return mode != MODE_GENERAL && unroll <= 2; }

// Which row walks zero-fill empty short rows on the side (GatherArgs::rider_ne): the plain sums with two-edge rounds.  An
// empty (node, type) bucket still needs its zero row, but not a lane group that walks short_rows -> rowptr -> out_row_map
// for it at the end of the launch, when no source row is being read any more: the group of a non-empty row sends those
// stores between issuing its first round of source-row loads and waiting for them.  MODE_GENERAL keeps one group per row
// (an empty max-row holds kFloatLowest, and its registers are tight), the per-head and edge-product walks and the rows that
// go two to a group (gather_rows_block_multi) likewise.
__host__ __device__ constexpr bool empty_riders(int mode, int unroll) { return mode == MODE_SUM && index_blocks(mode, unroll); }
struct NoRiders {
  __device__ __forceinline__ void operator()() const {}
};

// plain sums: the source rows of the round of edges [e, e + UNROLL) (part of one index block: UNROLL divides LPR and rounds
// start at multiples of UNROLL from the first edge).  Edges past `end` are not loaded (the walk of the other modes re-reads
// the last edge of an odd row).  `riders` is called once, behind the loads of the round's first edge.
template <int LPR, int VPL, int VEC, int UNROLL, class Riders = NoRiders>
__device__ __forceinline__ void issue_round(const GatherArgs& a, EdgeBlocks<LPR, MODE_SUM>& blocks, int32_t e, int32_t end, int f0,
                                            const bool (&live)[VPL], typename VecT<VEC>::type (&v)[UNROLL][VPL], float (&w)[UNROLL],
                                            const Riders& riders = Riders()) {
  static_assert(LPR % UNROLL == 0, "a round must not straddle two index blocks");
  if (e >= end) {
    riders();
    return;
  }
  blocks.seek(a, e);
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const int32_t idx = blocks.idx(e + u);
    w[u] = a.ew ? blocks.w(e + u) : 1.f;
    if (e + u < end) {
      const float* src = a.in + (int64_t)idx * a.ld_in + f0;
#pragma unroll
      for (int i = 0; i < VPL; ++i)
        if (live[i]) v[u][i] = vload<VEC>(src + i * LPR * VEC);
    }
    if (u == 0) riders();
  }
}
template <int LPR, int VPL, int VEC, int UNROLL>
__device__ __forceinline__ void add_round(int32_t e, int32_t end, const bool (&live)[VPL], const typename VecT<VEC>::type (&v)[UNROLL][VPL],
                                          const float (&w)[UNROLL], float (&acc)[VPL][VEC]) {
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    if (e + u < end) {
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        if (live[i]) {
          float x[VEC];
          vunpack<VEC>(v[u][i], x);
#pragma unroll
          for (int c = 0; c < VEC; ++c) {
            float m = w[u] * x[c];
            acc[i][c] += m;
          }
        }
      }
    }
  }
}

// accumulate edges [beg, end) into acc (lane-private chunks).  `riders` (row walks with empty_riders only): the zero-fill of
// the empty rows that ride with the lane group.  It runs once, in the first round, when the source row of the first edge has
// been asked for and nothing waits for it yet: the stores leave while that row is on its way.  They stand before the loads of
// the round's second edge, whose registers are still free there - behind the whole round the SP16 kernel at width 320 needs
// 108 registers instead of 90 and loses a wave per SIMD (NOTEBOOK section 48).
template <int LPR, int VPL, int VEC, int UNROLL, int MODE, class Riders = NoRiders>
__device__ __forceinline__ void accumulate_edges(const GatherArgs& a, int32_t beg, int32_t end, int f0,
                                                 const bool (&live)[VPL], float (&acc)[VPL][VEC], int64_t row,
                                                 const Riders& riders = Riders()) {
  using V = typename VecT<VEC>::type;
  EdgeBlocks<LPR, MODE> blocks;
  if constexpr (index_blocks(MODE, UNROLL)) blocks.start(a, beg, end);
  if constexpr (MODE == MODE_SUM && index_blocks(MODE, UNROLL)) {
    // (loading the rows of round n + 1 before the adds of round n - whole rounds at 3 waves per SIMD, half rounds at 5 - was
    // slower than this loop at width 320: NOTEBOOK section 46)
    V v[UNROLL][VPL];
    float w[UNROLL];
    int32_t e = beg;
    if constexpr (!std::is_same<Riders, NoRiders>::value) {  // the first round, with the riders in it
      issue_round<LPR, VPL, VEC, UNROLL>(a, blocks, e, end, f0, live, v, w, riders);
      add_round<LPR, VPL, VEC, UNROLL>(e, end, live, v, w, acc);
      e += UNROLL;
    }
    for (; e < end; e += UNROLL) {
      issue_round<LPR, VPL, VEC, UNROLL>(a, blocks, e, end, f0, live, v, w);
      add_round<LPR, VPL, VEC, UNROLL>(e, end, live, v, w, acc);
    }
    return;
  }
  const bool is_max = MODE == MODE_GENERAL && a.is_max;
  int hidx[VPL];
  if (mode_heads(MODE)) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) hidx[i] = live[i] ? (f0 + i * LPR * VEC) / a.head_width : 0;
  }
  float yv[VPL][VEC];
  bool dot_writer = false;
  if constexpr (MODE == MODE_HEADS_DOT) {
    const float* yrow = a.dot_rows + row * a.ld_dot + f0;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
#pragma unroll
      for (int c = 0; c < VEC; ++c) yv[i][c] = 0.f;
      if (live[i]) vunpack<VEC>(vload<VEC>(yrow + i * LPR * VEC), yv[i]);
    }
    dot_writer = ((threadIdx.x % LPR) & ((1 << a.dot_lph_log2) - 1)) == 0;
  }
  // the split reduction (one store per edge instead of one per chunk) when the chunk count is 2 or 4 and a head has at
  // least that many lanes
  constexpr bool CAN_SPLIT = MODE == MODE_HEADS_DOT && (VPL == 2 || VPL == 4);
  const bool split = CAN_SPLIT && (1 << a.dot_lph_log2) >= VPL;
  bool split_writer = false;
  int split_head = 0;
  if (split) {  // which value the lane ends up with (dpp_split_sum), fixed per lane
    constexpr int SPLIT_BITS = VPL == 4 ? 2 : 1;
    const int lane = threadIdx.x % LPR;
    const int which = (lane >> (a.dot_lph_log2 - SPLIT_BITS)) & (VPL - 1);
    const int f = f0 + which * LPR * VEC;
    // copies sit in the lanes that differ in the bits below the splitting ones: the lane with those bits clear writes
    split_writer = (lane & ((1 << (a.dot_lph_log2 - SPLIT_BITS)) - 1)) == 0 && f < a.width;
    split_head = f / a.head_width;
  }
  for (int32_t e = beg; e < end; e += UNROLL) {
    int32_t idx[UNROLL];
    int32_t eid[UNROLL];
    int32_t dpos[UNROLL];
    float w[UNROLL];
    bool ok[UNROLL];
    if constexpr (index_blocks(MODE, UNROLL)) blocks.seek(a, e);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      int32_t ee = e + u;
      ok[u] = ee < end;
      ee = ok[u] ? ee : end - 1;  // (in the block of e: e <= end - 1 < e + u)
      eid[u] = ee;
      if constexpr (index_blocks(MODE, UNROLL)) {
        static_assert(LPR % UNROLL == 0, "a round must not straddle two index blocks");
        idx[u] = blocks.idx(ee);
        if constexpr (MODE == MODE_HEADS_DOT) dpos[u] = blocks.pos(ee);
        w[u] = (!mode_heads(MODE) && a.ew) ? blocks.w(ee) : 1.f;
      } else {
        idx[u] = a.col[ee];
        if constexpr (MODE == MODE_HEADS_DOT) dpos[u] = a.dot_pos ? a.dot_pos[ee] : ee;
        w[u] = (!mode_heads(MODE) && a.ew) ? a.ew[ee] : 1.f;
      }
    }
    V v[UNROLL][VPL];
    float wh[UNROLL][VPL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const float* src = a.in + (int64_t)idx[u] * a.ld_in + f0;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        if (live[i]) {
          v[u][i] = vload<VEC>(src + i * LPR * VEC);
          if (mode_heads(MODE)) wh[u][i] = a.ew[(int64_t)eid[u] * a.ew_heads + hidx[i]];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (ok[u]) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          if (live[i]) {
            float x[VEC];
            vunpack<VEC>(v[u][i], x);
            const float wt = mode_heads(MODE) ? wh[u][i] : w[u];
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
              float m = wt * x[c];
              if (MODE == MODE_GENERAL) {
                m = act_apply(a.pre_act, m);
                acc[i][c] = is_max ? fmaxf(acc[i][c], m) : acc[i][c] + m;
              } else {
                acc[i][c] += m;
              }
            }
          }
        }
      }
    }
    if constexpr (MODE == MODE_HEADS_DOT) {
      // all lanes of a row group walk the same edges, so the exchange is convergent inside the group (DPP moves data inside
      // a 16-lane row only; other groups of the wave may sit in another iteration, their lanes are not read)
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t pos = dpos[u];
        float p[VPL];
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          p[i] = 0.f;
          if (live[i]) {
            float x[VEC];
            vunpack<VEC>(v[u][i], x);
#pragma unroll
            for (int c = 0; c < VEC; ++c) p[i] += x[c] * yv[i][c];
          }
        }
        if constexpr (CAN_SPLIT) {
          if (split) {
            const int lane = threadIdx.x % LPR;
            int which = 0;
            float r = 0.f;
            switch (a.dot_lph_log2) {  // (wave-uniform)
              case 1: if constexpr (VPL <= 2) r = dpp_split_sum<VPL, 1>(p, lane, which); break;
              case 2: r = dpp_split_sum<VPL, 2>(p, lane, which); break;
              case 3: r = dpp_split_sum<VPL, 3>(p, lane, which); break;
              default: r = dpp_split_sum<VPL, 4>(p, lane, which); break;
            }
            if (ok[u] && split_writer) a.dot_out[pos * a.ew_heads + split_head] = r;
            continue;
          }
        }
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const float r = dpp_group_sum(p[i], a.dot_lph_log2);
          if (ok[u] && live[i] && dot_writer) a.dot_out[pos * a.ew_heads + hidx[i]] = r;
        }
      }
    }
  }
}

// the reduced row of a lane group (acc: the lane's chunks) -> output row orow: times the row's scale, then the SP16 bytes
// and scale, or the activation and the fp32 row
template <int LPR, int VPL, int VEC, int MODE, bool SP>
__device__ __forceinline__ void store_group_row(const GatherArgs& a, float (&acc)[VPL][VEC], const bool (&live)[VPL], float rs,
                                                int64_t orow, int f0, int gl, bool is_max, bool nonempty) {
  if constexpr (SP) {  // VEC == 4, one window: the lane group holds the whole row
    unsigned mx = 0u;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
#pragma unroll
      for (int c = 0; c < VEC; ++c) {
        acc[i][c] *= rs;
        if (live[i]) mx = sp_absmax_bits(mx, acc[i][c]);
      }
    const float sc = sp_row_scale<LPR>(a, mx, orow, gl == 0);
    uint8_t* drow = a.out_sp + orow * a.ld_out_sp;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if (live[i]) sp_store4(drow, f0 + i * LPR * VEC, make_float4(acc[i][0], acc[i][VEC > 1 ? 1 : 0], acc[i][VEC > 2 ? 2 : 0], acc[i][VEC > 3 ? 3 : 0]), sc);
    return;
  }
  float* dst = a.out + orow * a.ld_out + f0;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    if (live[i]) {
      float o[VEC];
#pragma unroll
      for (int c = 0; c < VEC; ++c) {
        float y = acc[i][c];
        // an empty max-segment keeps the lowest float (tf.math.unsorted_segment_max); scaling it
        // would overflow to -inf, so the scale only touches real results
        if (!is_max || nonempty) y *= rs;
        o[c] = act_apply(a.post_act, y);
      }
      vstore<VEC>(dst + i * LPR * VEC, o);
    }
  }
}

// The empty short rows that ride with the lane group of non-empty slot `slot` (empty_riders): slots slot + rider_ne,
// slot + 2 * rider_ne, .. of the list.  start() reads the first one's output row and scale next to the group's own opening
// loads; store_all() writes, for each of them, what a group of its own stores for a row without an edge (zero sums times the
// row's scale through the same epilogue, nothing where the row has no output row) and reads the next one's.
template <int LPR, int VPL, int VEC, int MODE, bool SP>
struct EmptyRiders {
  int64_t slot;
  int32_t orow;
  float rs;
  bool any;
  __device__ __forceinline__ void load(const GatherArgs& a) {
    any = slot < a.num_short;
    if (any) {
      const int32_t r = a.short_rows[slot];
      orow = a.out_row_map ? a.out_row_map[r] : r;
      rs = a.row_scale ? a.row_scale[r] : 1.f;
    }
  }
  __device__ __forceinline__ void start(const GatherArgs& a, int64_t own_slot) {
    slot = own_slot + a.rider_ne;
    orow = -1;
    rs = 1.f;
    any = false;
    if (a.rider_ne > 0) load(a);
  }
  __device__ __forceinline__ void store_all(const GatherArgs& a, const bool (&live)[VPL], int f0, int gl) {
    while (any) {
      if (orow >= 0) {
        float zero[VPL][VEC];
#pragma unroll
        for (int i = 0; i < VPL; ++i)
#pragma unroll
          for (int c = 0; c < VEC; ++c) zero[i][c] = 0.f;
        store_group_row<LPR, VPL, VEC, MODE, SP>(a, zero, live, rs, orow, f0, gl, false, false);
      }
      slot += a.rider_ne;
      load(a);
    }
  }
};

template <int LPR, int VPL, int VEC, int UNROLL, int MODE, bool SP = false>
__device__ __forceinline__ void gather_rows_block(const GatherArgs& a, unsigned row_block, unsigned window) {
  constexpr int GROUPS_PER_BLOCK = 256 / LPR;
  constexpr int WINDOW = LPR * VPL * VEC;  // floats covered per pass
  constexpr bool RIDERS = empty_riders(MODE, UNROLL);
  const int tid = threadIdx.x;
  const int group = tid / LPR;
  const int gl = tid % LPR;
  const int64_t slot = (int64_t)row_block * GROUPS_PER_BLOCK + group;
  if (slot >= ((RIDERS && a.rider_ne > 0) ? a.rider_ne : a.short_rows ? a.num_short : a.num_rows)) return;
  const int64_t row = a.short_rows ? a.short_rows[slot] : slot;
  EmptyRiders<LPR, VPL, VEC, MODE, SP> riders;
  if constexpr (RIDERS) riders.start(a, slot);
  const int f0 = window * WINDOW + gl * VEC;  // first float of this lane's chunk 0
  const int32_t beg = a.rowptr[row];
  const int32_t end = a.rowptr[row + 1];
  // (with riders, rider_ne > 0, neither happens: the slots below rider_ne hold short rows of a view with a row for every bucket)
  if (a.long_threshold > 0 && end - beg > a.long_threshold) return;  // handled by the item kernels
  const int64_t orow = a.out_row_map ? a.out_row_map[row] : row;
  if (orow < 0) return;  // compact output: empty buckets have no row
  const bool is_max = MODE == MODE_GENERAL && a.is_max;

  float acc[VPL][VEC];
  bool live[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    live[i] = (f0 + i * LPR * VEC) < a.width;
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[i][c] = is_max ? kFloatLowest : 0.f;
  }
  if constexpr (RIDERS)
    accumulate_edges<LPR, VPL, VEC, UNROLL, MODE>(a, beg, end, f0, live, acc, row, [&]() { riders.store_all(a, live, f0, gl); });
  else
    accumulate_edges<LPR, VPL, VEC, UNROLL, MODE>(a, beg, end, f0, live, acc, row);

  const float rs = a.row_scale ? a.row_scale[row] : 1.f;
  store_group_row<LPR, VPL, VEC, MODE, SP>(a, acc, live, rs, orow, f0, gl, is_max, end > beg);
}

// Short rows (round 6): a lane group takes R rows AT ONCE and walks them side by side, U edges of each per round.  A bucket of
// a molecule batch holds 0 - 4 edges: with one row per group the chain of dependent loads (row list -> row pointers -> columns
// -> source rows) is walked once per row with at most its own few source rows in flight at the end - the node-view gathers of
// the per-edge messages of configs[3] moved 2.3 GB in 0.83 ms (0.35 of the HBM peak) with every CU full of waiting waves.
// Here the R chains of a group advance together (R x U x VPL 16-byte loads in flight per lane) and loads past the end of a row
// are not issued (the one-row walk re-reads the row's last edge up to UNROLL - 1 times).  Every row still adds its edges in CSR
// order with the same arithmetic: results are bit-identical to gather_rows_block.  MODE_SUM, one feature window.
template <int LPR, int VPL, int VEC, bool SP, int R, int U>
__device__ __forceinline__ void gather_rows_block_multi(const GatherArgs& a, unsigned row_block) {
  using V = typename VecT<VEC>::type;
  constexpr int GROUPS_PER_BLOCK = 256 / LPR;
  const int tid = threadIdx.x;
  const int group = tid / LPR;
  const int gl = tid % LPR;
  const int64_t nslots = a.short_rows ? a.num_short : a.num_rows;
  const int64_t slot0 = (int64_t)row_block * (GROUPS_PER_BLOCK * R) + group;  // row r of the group: slot0 + r * GROUPS_PER_BLOCK
  const int f0 = gl * VEC;
  bool live[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) live[i] = (f0 + i * LPR * VEC) < a.width;
  int64_t row[R];
  bool on[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t slot = slot0 + (int64_t)r * GROUPS_PER_BLOCK;
    on[r] = slot < nslots;
    row[r] = on[r] ? (a.short_rows ? (int64_t)a.short_rows[slot] : slot) : 0;
  }
  int32_t beg[R], len[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    beg[r] = a.rowptr[row[r]];
    len[r] = a.rowptr[row[r] + 1] - beg[r];
  }
  int64_t orow[R];
  float rs[R];
  int32_t maxlen = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    orow[r] = a.out_row_map ? (int64_t)a.out_row_map[row[r]] : row[r];
    rs[r] = a.row_scale ? a.row_scale[row[r]] : 1.f;
    // (rows of the item kernels; compact output: empty buckets have no row)
    if ((a.long_threshold > 0 && len[r] > a.long_threshold) || orow[r] < 0) on[r] = false;
    if (!on[r]) len[r] = 0;
    maxlen = len[r] > maxlen ? len[r] : maxlen;
  }
  float acc[R][VPL][VEC];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int i = 0; i < VPL; ++i)
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[r][i][c] = 0.f;

  for (int32_t j = 0; j < maxlen; j += U) {
    int32_t idx[R][U];
    float w[R][U];
    bool ok[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ok[r][u] = j + u < len[r];
        idx[r][u] = 0;
        w[r][u] = 1.f;
        if (ok[r][u]) {
          const int32_t e = beg[r] + j + u;
          idx[r][u] = a.col[e];
          if (a.ew) w[r][u] = a.ew[e];
        }
      }
    V v[R][U][VPL];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[r][u]) {
          const float* src = a.in + (int64_t)idx[r][u] * a.ld_in + f0;
#pragma unroll
          for (int i = 0; i < VPL; ++i)
            if (live[i]) v[r][u][i] = vload<VEC>(src + i * LPR * VEC);
        }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[r][u]) {
#pragma unroll
          for (int i = 0; i < VPL; ++i)
            if (live[i]) {
              float x[VEC];
              vunpack<VEC>(v[r][u][i], x);
#pragma unroll
              for (int c = 0; c < VEC; ++c) {
                float m = w[r][u] * x[c];
                acc[r][i][c] += m;
              }
            }
        }
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!on[r]) continue;
    if constexpr (SP) {
      unsigned mx = 0u;
#pragma unroll
      for (int i = 0; i < VPL; ++i)
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          acc[r][i][c] *= rs[r];
          if (live[i]) mx = sp_absmax_bits(mx, acc[r][i][c]);
        }
      const float sc = sp_row_scale<LPR>(a, mx, orow[r], gl == 0);
      uint8_t* drow = a.out_sp + orow[r] * a.ld_out_sp;
#pragma unroll
      for (int i = 0; i < VPL; ++i)
        if (live[i])
          sp_store4(drow, f0 + i * LPR * VEC,
                    make_float4(acc[r][i][0], acc[r][i][VEC > 1 ? 1 : 0], acc[r][i][VEC > 2 ? 2 : 0], acc[r][i][VEC > 3 ? 3 : 0]), sc);
    } else {
      float* dst = a.out + orow[r] * a.ld_out + f0;
#pragma unroll
      for (int i = 0; i < VPL; ++i)
        if (live[i]) {
          float o[VEC];
#pragma unroll
          for (int c = 0; c < VEC; ++c) o[c] = act_apply(a.post_act, acc[r][i][c] * rs[r]);
          vstore<VEC>(dst + i * LPR * VEC, o);
        }
    }
  }
}

// ---- rows made of several items -------------------------------------------------------------------------------------------
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
// 16 bytes of partial row `slot` at float c, read past this XCD's caches (sc1): every load of a partial row goes this way
__device__ __forceinline__ float4 load_partial4(const GatherArgs& a, int64_t slot, int c) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.partial + slot * a.width, (short)0, a.width * 4, 0x00020000);
  const uint4v v = __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)c * 4u, 0, 16 /* sc1 */);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ float load_partial1(const GatherArgs& a, int64_t slot, int f) {
  return __hip_atomic_load(a.partial + slot * a.width + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The partial rows of a multi-item row (scratch slots base, base + 1, .. base + n - 1) -> its SP16 row: ONE WAVE, lane = its
// lane (width <= 2048 floats).  Sums in item order, four partial rows in flight.
__device__ __forceinline__ void combine_sp_row(const GatherArgs& a, int64_t row, int32_t base, int32_t n, float rs, int lane) {
  float4 sum[8];
  unsigned mx = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = (lane + i * 64) * 4;
    sum[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < a.width) {
      int k = 0;
      for (; k + 4 <= n; k += 4) {  // four partial rows in flight; the sum stays in item order
        float4 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = load_partial4(a, base + k + u, c);
#pragma unroll
        for (int u = 0; u < 4; ++u) { sum[i].x += p[u].x; sum[i].y += p[u].y; sum[i].z += p[u].z; sum[i].w += p[u].w; }
      }
      for (; k < n; ++k) {
        const float4 p = load_partial4(a, base + k, c);
        sum[i].x += p.x; sum[i].y += p.y; sum[i].z += p.z; sum[i].w += p.w;
      }
      sum[i].x *= rs; sum[i].y *= rs; sum[i].z *= rs; sum[i].w *= rs;
      mx = sp_absmax_bits(sp_absmax_bits(sp_absmax_bits(sp_absmax_bits(mx, sum[i].x), sum[i].y), sum[i].z), sum[i].w);
    }
  }
  const int64_t orow = a.out_row_map ? a.out_row_map[row] : row;
  float iv, sc;
  if (a.fixed_inv) {
    iv = a.fixed_inv[0];
    sc = 1.f / iv;
  } else {
#pragma unroll
    for (int o = 32; o; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
    sc = sp_scale_for_max(__uint_as_float(mx), &iv);
    if (lane == 0) a.inv_out[orow] = iv;
  }
  uint8_t* drow = a.out_sp + orow * a.ld_out_sp;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = (lane + i * 64) * 4;
    if (c < a.width) sp_store4(drow, c, sum[i], sc);
  }
}

// ... -> floats [f0, f1) of its fp32 row: the whole workgroup, one float per thread and round
__device__ __forceinline__ void combine_fp32_row(const GatherArgs& a, int64_t row, int32_t base, int32_t n, float rs, bool is_max,
                                                 int f0, int f1) {
  const int64_t orow = a.out_row_map ? a.out_row_map[row] : row;
  for (int f = f0 + (int)threadIdx.x; f < f1; f += 256) {
    float s = load_partial1(a, base, f);
    for (int k = 1; k < n; ++k) {
      const float p = load_partial1(a, base + k, f);
      s = is_max ? fmaxf(s, p) : s + p;
    }
    a.out[orow * a.ld_out + f] = act_apply(a.post_act, s * rs);
  }
}

// Called by every thread of an item workgroup that has just stored its partial row (slot >= 0), once per launch and
// (item, feature window).  The hand-off between the workgroups of a row - they run on any CU of any XCD, and the XCDs' L2s
// are not coherent for plain stores - is the one the K split inside the NT product uses (gemm_sp.hip):
//   the partial rows are stored write-through (sc1); every wave waits for its stores, the workgroup meets at a barrier, and
//   thread 0 adds 1 to the row's counter (agent scope); the workgroup that draws the last ticket sets the counter back to 0
//   for the next launch and reads all partial rows of the row with loads that go past its own caches (sc1, every one of them).
// No cache is written back or invalidated as a whole (a release / acquire fence pair at agent scope does both, in the middle
// of a launch that streams 150 MB through the L2s: measured 9 us per gather, NOTEBOOK section 23).  Nobody waits for
// anybody: a workgroup that is not the last one leaves.  Feature window w counts on counter w % ARRIVE_WINDOWS of the row;
// with more windows than counters the windows of one residue class share a counter and the last of THEIR item workgroups
// finishes all of them.  `flag`: one word of the workgroup's LDS array (free by now).
template <int WINDOW, bool SP>
__device__ __forceinline__ void finish_multi_row(const GatherArgs& a, int item, int64_t row, float rs, unsigned window, bool is_max,
                                                 unsigned* flag) {
  const int m = a.item_multi[item];
  const int32_t n = a.multi_n[m];
  const unsigned windows = gridDim.y;
  const unsigned cls = window % ARRIVE_WINDOWS;
  const unsigned sharing = (windows - cls + ARRIVE_WINDOWS - 1) / ARRIVE_WINDOWS;  // windows cls, cls + ARRIVE_WINDOWS, ..
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's partial stores have left
  __syncthreads();                                   // ... every wave's (and every read of the LDS array is over)
  if (threadIdx.x == 0) {
    uint32_t* ctr = a.arrive + (size_t)m * ARRIVE_WINDOWS + cls;
    const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = old == (unsigned)n * sharing - 1u;
    if (last) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // all tickets of this launch are drawn
    *flag = last ? 1u : 0u;
  }
  __syncthreads();
  if (*flag == 0u) return;
  const int32_t base = a.multi_base[m];
  if constexpr (SP) {  // (one feature window)
    if (threadIdx.x < 64) combine_sp_row(a, row, base, n, rs, (int)threadIdx.x);
  } else {
    for (unsigned w = cls; w < windows; w += ARRIVE_WINDOWS)
      combine_fp32_row(a, row, base, n, rs, is_max, (int)(w * WINDOW), min(a.width, (int)((w + 1) * WINDOW)));
  }
}

// one workgroup per item (a run of <= item_chunk_edges edges of a long row)
template <int LPR, int VPL, int VEC, int UNROLL, int MODE, bool SP = false>
__device__ __forceinline__ void gather_item_block(const GatherArgs& a, int item, unsigned window,
                                                  float (&red)[256 / LPR][LPR * VPL * VEC]) {
  constexpr int GROUPS = 256 / LPR;
  constexpr int WINDOW = LPR * VPL * VEC;
  const int tid = threadIdx.x;
  const int group = tid / LPR;
  const int gl = tid % LPR;
  const int64_t row = a.item_row[item];
  const int32_t rbeg = a.rowptr[row], rend = a.rowptr[row + 1];
  const int32_t ibeg = rbeg + a.item_chunk[item] * a.item_chunk_edges;
  const int32_t iend = min(rend, ibeg + a.item_chunk_edges);
  // the item's edges are dealt evenly to the lane groups (in pairs: the walk is unrolled by UNROLL), so a
  // 60-edge row keeps all 16 groups busy instead of the first five
  int per = (iend - ibeg + GROUPS - 1) / GROUPS;
  per = (per + UNROLL - 1) / UNROLL * UNROLL;
  const int32_t beg = min(iend, ibeg + group * per);
  const int32_t end = min(iend, beg + per);
  const int w0 = window * WINDOW;
  const int f0 = w0 + gl * VEC;
  const bool is_max = MODE == MODE_GENERAL && a.is_max;

  float acc[VPL][VEC];
  bool live[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    live[i] = (f0 + i * LPR * VEC) < a.width;
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[i][c] = is_max ? kFloatLowest : 0.f;
  }
  accumulate_edges<LPR, VPL, VEC, UNROLL, MODE>(a, beg, end, f0, live, acc, row);
#pragma unroll
  for (int i = 0; i < VPL; ++i)
#pragma unroll
    for (int c = 0; c < VEC; ++c) red[group][(gl + i * LPR) * VEC + c] = acc[i][c];
  __syncthreads();
  const int32_t slot = a.item_slot[item];
  const float rs = a.row_scale ? a.row_scale[row] : 1.f;
  if constexpr (SP) {
    if (slot < 0) {  // the item is the whole row: sums -> red[0], row maximum, split store
      unsigned mx = 0u;  // (sp_absmax_bits)
      for (int f = tid; f < WINDOW; f += 256) {
        if (w0 + f >= a.width) break;
        float v = red[0][f];
#pragma unroll
        for (int g = 1; g < GROUPS; ++g) v += red[g][f];
        v *= rs;
        red[0][f] = v;
        mx = sp_absmax_bits(mx, v);
      }
#pragma unroll
      for (int o = 32; o; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
      __syncthreads();  // every sum over red[1..] has been taken
      if ((tid & 63) == 0) red[1][tid >> 6] = __uint_as_float(mx);
      __syncthreads();
      mx = max(max(__float_as_uint(red[1][0]), __float_as_uint(red[1][1])), max(__float_as_uint(red[1][2]), __float_as_uint(red[1][3])));
      const int64_t orow = a.out_row_map ? a.out_row_map[row] : row;
      float iv, sc;
      if (a.fixed_inv) {
        iv = a.fixed_inv[0];
        sc = 1.f / iv;
      } else {
        sc = sp_scale_for_max(__uint_as_float(mx), &iv);
        if (tid == 0) a.inv_out[orow] = iv;
      }
      uint8_t* drow = a.out_sp + orow * a.ld_out_sp;
      for (int c4 = tid; c4 * 4 < WINDOW; c4 += 256)
        if (w0 + c4 * 4 < a.width)
          sp_store4(drow, w0 + c4 * 4, make_float4(red[0][c4 * 4], red[0][c4 * 4 + 1], red[0][c4 * 4 + 2], red[0][c4 * 4 + 3]), sc);
      return;
    }
  }
  for (int f = tid; f < WINDOW; f += 256) {
    if (w0 + f >= a.width) break;
    float s = red[0][f];
#pragma unroll
    for (int g = 1; g < GROUPS; ++g) s = is_max ? fmaxf(s, red[g][f]) : s + red[g][f];
    if (slot < 0) {
      const int64_t orow = a.out_row_map ? a.out_row_map[row] : row;
      a.out[orow * a.ld_out + w0 + f] = act_apply(a.post_act, s * rs);
    } else {
      // write-through (sc1): the row's last-arriving workgroup may sit on another XCD, whose L2 never sees a plain store
      __hip_atomic_store(a.partial + (int64_t)slot * a.width + w0 + f, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (slot >= 0) finish_multi_row<WINDOW, SP>(a, item, row, rs, window, is_max, reinterpret_cast<unsigned*>(&red[0][0]));
}

// One launch covers both kinds of work: workgroups [0, num_items) each take one item of a long row
// (longest work first), the remaining workgroups take 256/LPR short rows each.
template <int LPR, int VPL, int VEC, int UNROLL, int MODE, bool SP = false>
__global__ void __launch_bounds__(256) csr_gather_reduce_kernel(GatherArgs a, int num_items) {
  __shared__ float red[256 / LPR][LPR * VPL * VEC];
  const unsigned unit = blockIdx.x, window = blockIdx.y;
  if ((int)unit < num_items)
    gather_item_block<LPR, VPL, VEC, UNROLL, MODE, SP>(a, (int)unit, window, red);
  else
    gather_rows_block<LPR, VPL, VEC, UNROLL, MODE, SP>(a, unit - (unsigned)num_items, window);
}

// the same launch with the short rows R to a lane group (one feature window, plain sums)
template <int LPR, int VPL, int VEC, int UNROLL, bool SP, int R, int U>
__global__ void __launch_bounds__(256) csr_gather_reduce_multi_kernel(GatherArgs a, int num_items) {
  __shared__ float red[256 / LPR][LPR * VPL * VEC];
  const unsigned unit = blockIdx.x;
  if ((int)unit < num_items)
    gather_item_block<LPR, VPL, VEC, UNROLL, MODE_SUM, SP>(a, (int)unit, 0, red);
  else
    gather_rows_block_multi<LPR, VPL, VEC, SP, R, U>(a, unit - (unsigned)num_items);
}

template <int LPR, int VPL, int VEC, int UNROLL, bool SP, int R, int U>
static void launch_multi(GatherArgs a, int num_items, hipStream_t s) {
  const unsigned units = (unsigned)(num_items + ceil_div(a.short_rows ? a.num_short : a.num_rows, (256 / LPR) * R));
  hipLaunchKernelGGL((csr_gather_reduce_multi_kernel<LPR, VPL, VEC, UNROLL, SP, R, U>), dim3(units, 1), dim3(256), 0, s, a, num_items);
}

template <int LPR, int VPL, int VEC, int UNROLL, int MODE, bool SP = false>
static int launch_mode(GatherArgs a, int num_items, hipStream_t s) {
  constexpr int GROUPS_PER_BLOCK = 256 / LPR;
  constexpr int WINDOW = LPR * VPL * VEC;
  const unsigned windows = (unsigned)ceil_div(a.width, WINDOW);
  if constexpr (!empty_riders(MODE, UNROLL)) a.rider_ne = 0;
  // (with riders the empty short rows have no lane group: row workgroups for the non-empty ones only)
  const unsigned units = (unsigned)(num_items + ceil_div(a.rider_ne > 0 ? a.rider_ne : a.short_rows ? a.num_short : a.num_rows, GROUPS_PER_BLOCK));
  dim3 block(256);
  bool multi_done = false;
  if constexpr (MODE == MODE_SUM && VEC == 4 && LPR * VPL <= 128) {
    if (a.multi_pairs && windows == 1 && (!SP || a.width <= 2048)) {
      launch_multi<LPR, VPL, VEC, UNROLL, SP, 2, 1>(a, num_items, s);
      multi_done = true;
    }
  }
  if constexpr (SP) {
    if (windows != 1 || a.width > 2048) {
      set_error("SP16 gather output needs the whole row in one feature window (width %d)", a.width);
      return TFGNN_ERR_UNSUPPORTED;
    }
    if (!multi_done)
      hipLaunchKernelGGL((csr_gather_reduce_kernel<LPR, VPL, VEC, UNROLL, MODE, true>), dim3(units, 1), block, 0, s, a, num_items);
    TFGNN_LAUNCH_CHECK();
    return TFGNN_OK;
  }
  if (!multi_done)
    hipLaunchKernelGGL((csr_gather_reduce_kernel<LPR, VPL, VEC, UNROLL, MODE>), dim3(units, windows), block, 0, s, a,
                       num_items);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}

template <int LPR, int VPL, int VEC, int UNROLL>
static int launch_variant(const GatherArgs& a, int mode, int num_items, hipStream_t s) {
  if (mode == MODE_SUM) return launch_mode<LPR, VPL, VEC, UNROLL, MODE_SUM>(a, num_items, s);
  if (mode == MODE_HEADS) return launch_mode<LPR, VPL, VEC, UNROLL, MODE_HEADS>(a, num_items, s);
  if (mode == MODE_HEADS_DOT) {
    if constexpr (VEC == 4) {
      TFGNN_REQUIRE((1 << a.dot_lph_log2) <= LPR, "fused edge products: a head is wider than a lane group (width %d)", a.width);
      return launch_mode<LPR, VPL, VEC, UNROLL, MODE_HEADS_DOT>(a, num_items, s);
    } else {
      set_error("fused edge products need 16-byte aligned rows");
      return TFGNN_ERR_UNSUPPORTED;
    }
  }
  return launch_mode<LPR, VPL, VEC, UNROLL, MODE_GENERAL>(a, num_items, s);
}

// average edges per walked row up to which the short rows go two to a lane group
constexpr double kMultiAvgLen = 1.5;

static int gather_dispatch(GatherArgs a, int num_items, hipStream_t s) {
  int mode = MODE_SUM;
  if (a.is_max || a.pre_act != TFGNN_ACT_NONE) mode = MODE_GENERAL;
  if (a.ew && a.ew_heads > 1) {
    TFGNN_REQUIRE(mode == MODE_SUM, "per-head edge weights only support plain sums");
    TFGNN_REQUIRE(a.head_width > 0 && a.width % a.head_width == 0 && a.width / a.head_width == a.ew_heads,
                  "width %d is not ew_heads %d x head_width %d", a.width, a.ew_heads, a.head_width);
    mode = MODE_HEADS;
    if (a.dot_out) {
      TFGNN_REQUIRE(a.dot_rows && a.ld_dot >= a.width && a.ld_dot % 4 == 0 && (uintptr_t)a.dot_rows % 16 == 0,
                    "fused edge products: bad row operand");
      mode = MODE_HEADS_DOT;
    }
  }
  TFGNN_REQUIRE(!a.dot_out || mode == MODE_HEADS_DOT, "fused edge products ride on the per-head weighted sums only");
  const bool vec4 = (a.width % 4 == 0) && (a.ld_in % 4 == 0) && (a.ld_out % 4 == 0) &&
                    (((uintptr_t)a.in | (uintptr_t)a.out) % 16 == 0) && (!a.out_sp || a.ld_out_sp % 64 == 0) &&
                    (!mode_heads(mode) || a.head_width % 4 == 0);
  TFGNN_REQUIRE(vec4 || !a.out_sp, "SP16 gather output needs 16-byte aligned rows");
  if (!vec4) {
    // scalar path (odd widths: unit tests, tiny models): 16 lanes x 4 floats per pass
    return launch_variant<16, 4, 1, 2>(a, mode, num_items, s);
  }
  const int chunks = a.width / 4;
  if (a.out_sp) {  // SP16 output: plain sums on the float4 path, whole rows per lane group
    TFGNN_REQUIRE(mode == MODE_SUM && a.width % 16 == 0, "SP16 gather output: plain sums of rows with width %% 16 == 0 only");
    if (chunks <= 8) return launch_mode<8, 1, 4, 8, MODE_SUM, true>(a, num_items, s);
    if (chunks <= 16) return launch_mode<16, 1, 4, 8, MODE_SUM, true>(a, num_items, s);
    if (chunks <= 32) return launch_mode<16, 2, 4, 4, MODE_SUM, true>(a, num_items, s);
    if (chunks <= 64) return launch_mode<16, 4, 4, 2, MODE_SUM, true>(a, num_items, s);
    if (chunks <= 80) return launch_mode<16, 5, 4, 2, MODE_SUM, true>(a, num_items, s);  // UNROLL 1 / 4 and 32 lanes per row measured slower (tools/gather_l2_probe.py)
    return launch_mode<32, 4, 4, 2, MODE_SUM, true>(a, num_items, s);
  }
  // (rows of 8 floats - RGAT's per-head logit gradients summed per bucket - leave six of the eight lanes of the next variant
  // idle; a two-lane variant measured SLOWER, 28 vs 23 us at configs[2]: the launch is bound by the walk along the rows)
  if (chunks <= 8) return launch_variant<8, 1, 4, 8>(a, mode, num_items, s);
  if (chunks <= 16) return launch_variant<16, 1, 4, 8>(a, mode, num_items, s);
  if (chunks <= 32) return launch_variant<16, 2, 4, 4>(a, mode, num_items, s);
  if (chunks <= 64) return launch_variant<16, 4, 4, 2>(a, mode, num_items, s);
  if (chunks % 80 == 0 || chunks <= 80) return launch_variant<16, 5, 4, 2>(a, mode, num_items, s);
  return launch_variant<32, 4, 4, 2>(a, mode, num_items, s);
}

static int check_common(int64_t num_rows, const void* rowptr, const void* in, const void* out, int64_t ld_in,
                        int64_t ld_out, int width, int reduce_op) {
  TFGNN_REQUIRE(rowptr && in && out, "NULL pointer");
  TFGNN_REQUIRE(ld_in >= width && ld_out >= width, "leading dimension smaller than width");
  TFGNN_REQUIRE(reduce_op == TFGNN_REDUCE_SUM || reduce_op == TFGNN_REDUCE_MAX, "unknown reduce op %d", reduce_op);
  TFGNN_REQUIRE(num_rows < ((int64_t)1 << 31), "too many rows");
  return TFGNN_OK;
}

}  // namespace tfgnn

extern "C" int tfgnn_csr_gather_reduce(const int32_t* d_rowptr, const int32_t* d_col,
                                       const float* d_edge_weight, const float* d_row_scale,
                                       int64_t num_rows, const float* d_in, int64_t ld_in, int width,
                                       float* d_out, int64_t ld_out, int reduce_op, int pre_act,
                                       int post_act, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(num_rows >= 0 && width >= 0, "negative size");
  if (num_rows == 0 || width == 0) return TFGNN_OK;
  int rc = check_common(num_rows, d_rowptr, d_in, d_out, ld_in, ld_out, width, reduce_op);
  if (rc) return rc;
  GatherArgs a{};
  a.rowptr = d_rowptr; a.col = d_col; a.ew = d_edge_weight; a.row_scale = d_row_scale;
  a.num_rows = num_rows; a.in = d_in; a.ld_in = ld_in; a.width = width; a.out = d_out; a.ld_out = ld_out;
  a.pre_act = pre_act; a.post_act = post_act; a.is_max = reduce_op == TFGNN_REDUCE_MAX;
  a.ew_heads = 1; a.head_width = width;
  return gather_dispatch(a, 0, (hipStream_t)stream);
}

extern "C" size_t tfgnn_graph_gather_workspace_bytes(const tfgnn_graph* g, int view, int width) {
  if (!g || view < 0 || view > 7 || width <= 0) return 0;
  if (view >= 4) view = (view == 4 || view == 6) ? 0 : 2;
  return (size_t)g->views[view].plan.num_partials * (size_t)width * 4;
}

extern "C" int tfgnn_graph_gather_dot_supported(int width, int ew_heads);
static int graph_gather_impl(const tfgnn_graph* g, int view, const int32_t* d_col_override,
                             const float* d_edge_weight, int ew_heads, const float* d_row_scale,
                             const float* d_in, int64_t ld_in, int width, float* d_out,
                             int64_t ld_out, int reduce_op, int pre_act, int post_act,
                             void* d_workspace, size_t workspace_bytes, void* stream, void* d_out_sp, int64_t ld_out_sp,
                             float* d_inv_scale, const float* d_fixed_inv, tfgnn_aux_job* combine_job = nullptr,
                             const float* d_dot_rows = nullptr, int64_t ld_dot = 0, const int32_t* d_dot_pos = nullptr,
                             float* d_dot_out = nullptr, bool keep_empty = false) {
  using namespace tfgnn;
  TFGNN_REQUIRE(g != nullptr, "graph is NULL");
  TFGNN_REQUIRE(view >= 0 && view <= 6, "unknown graph view %d", view);
  TFGNN_REQUIRE(width >= 0 && ew_heads >= 1, "bad sizes");
  // views 4 / 5: the typed views 0 / 2 with compact output (one row per NON-EMPTY bucket, type-major)
  {
    unsigned need = (view == 1 || view == 3) ? TFGNN_GRAPH_PART_PLAN_NODE : TFGNN_GRAPH_PART_PLAN_TYPED;
    if (view == 4 || view == 5) need |= TFGNN_GRAPH_PART_COMPACT;
    if (view == 6) need |= TFGNN_GRAPH_PART_DST_PATTERN;
    const int prc = graph_require_parts(g, need, "tfgnn_graph_gather_reduce");
    if (prc) return prc;
  }
  const int32_t* out_map = nullptr;
  int64_t compact_nz = -1;
  if (view == 6) {  // by-target buckets, rows in pattern order
    TFGNN_REQUIRE(g->L <= 8, "TFGNN_VIEW_BY_DST_TYPED_PATTERN: at most 8 edge types");
    out_map = g->pat_rowmap_d;
    view = 0;
  } else if (view >= 4) {
    out_map = g->compact[view - 4].cpos;
    compact_nz = g->compact[view - 4].num_nz;
    view = view == 4 ? 0 : 2;
  }
  const GraphView& gv = g->views[view];
  if (gv.num_rows == 0 || width == 0) return TFGNN_OK;
  int rc = check_common(gv.num_rows, gv.rowptr, d_in, d_out_sp ? (const void*)d_out_sp : (const void*)d_out, ld_in,
                        d_out_sp ? (int64_t)width : ld_out, width, reduce_op);
  if (rc) return rc;
  const CsrPlan& p = gv.plan;
  TFGNN_REQUIRE(p.num_partials == 0 || (d_workspace && workspace_bytes >= (size_t)p.num_partials * width * 4),
                "workspace too small: need %zu bytes", (size_t)p.num_partials * width * 4);
  GatherArgs a{};
  a.rowptr = gv.rowptr; a.col = d_col_override ? d_col_override : gv.col; a.ew = d_edge_weight;
  a.row_scale = d_row_scale; a.num_rows = gv.num_rows; a.in = d_in; a.ld_in = ld_in; a.width = width;
  a.out = d_out; a.ld_out = d_out_sp ? (int64_t)width : ld_out; a.pre_act = pre_act; a.post_act = post_act;
  a.out_sp = (uint8_t*)d_out_sp; a.ld_out_sp = ld_out_sp; a.inv_out = d_inv_scale; a.fixed_inv = d_fixed_inv;
  if (combine_job) memset(combine_job, 0, sizeof(*combine_job));  // (kind 0: the gather combines its long rows itself)
  a.is_max = reduce_op == TFGNN_REDUCE_MAX; a.ew_heads = ew_heads; a.head_width = width / ew_heads;
  a.long_threshold = p.long_threshold;
  a.out_row_map = out_map;
  if (d_dot_out) {
    TFGNN_REQUIRE(ew_heads > 1 && d_edge_weight && width % ew_heads == 0, "tfgnn_graph_gather_reduce_dot: per-head edge weights only");
    const int lph = width / ew_heads / 4;
    TFGNN_REQUIRE(tfgnn_graph_gather_dot_supported(width, ew_heads), "tfgnn_graph_gather_reduce_dot: unsupported head width %d",
                  width / ew_heads);
    a.dot_rows = d_dot_rows; a.ld_dot = ld_dot; a.dot_out = d_dot_out; a.dot_pos = d_dot_pos;
    a.dot_lph_log2 = 31 - __builtin_clz((unsigned)lph);
  }
  a.item_row = p.item_row; a.item_chunk = p.item_chunk; a.item_slot = p.item_slot; a.item_multi = p.item_multi;
  a.partial = (float*)d_workspace; a.item_chunk_edges = p.item_chunk_edges;
  a.multi_base = p.multi_base; a.multi_n = p.multi_n; a.arrive = p.arrive;
  a.short_rows = p.short_rows;
  a.num_short = p.num_short;
  // compact output: the empty buckets have no row, and they close the length-ordered list - no lane groups for them
  // (configs[4]: 452 517 of 6.8 M by-source buckets are non-empty; walking all of them was 0.85 M workgroups with nothing to do)
  if (compact_nz >= 0) a.num_short = std::max<int64_t>(0, (int64_t)p.num_short - (gv.num_rows - compact_nz));
  // every other output has a zero row for an empty bucket: written by the lane groups of the non-empty short rows, which the
  // list holds first (the walks with empty_riders; launch_mode sets it back for the others)
  else if (a.short_rows && p.num_empty > 0 && p.num_short > p.num_empty) a.rider_ne = (int64_t)p.num_short - p.num_empty;
  // ... unless the caller vouches that the operand already holds them (tfgnn_graph_gather_reduce_sp_keep_empty): the empty rows
  // close the list, so the launch ends in front of them - no lane group, no rider, no store for any of them.  Per-row scales
  // only: an empty row's scale is the marker, whatever the tensor-wide one would be
  const bool keep = keep_empty && compact_nz < 0 && d_out_sp && d_inv_scale && !d_fixed_inv && a.short_rows && p.num_empty > 0;
  {
    // short rows side by side (gather_rows_block_multi) when the rows the row workgroups walk hold <= 1.5 edges on average -
    // the (node, type) buckets of a molecule batch (0.6): tools/gather_short_probe.py, 128k molecules, H = 128: typed by-target
    // view 1109 -> 948 us, typed by-source view with SP16 output 1257 -> 1132 us with two rows per group and one edge of each
    // per round; four rows, or two edges per round: 1070 - 1277 / 1156 - 1306 us; a persistent grid (4 - 16 workgroups per CU
    // walking the units): no better.  The node views (3 edges per row) run at 5.0 - 5.2 TB/s either way and keep one row per
    // group.  TFGNN_GATHER_MULTI = 1: off; 21: every plain-sum launch (tests)
    const char* multi_env = getenv("TFGNN_GATHER_MULTI");  // (read per call: the tests compare the two shapes in one process)
    const int multi_knob = multi_env ? atoi(multi_env) : 0;
    const int64_t nslots = a.short_rows ? a.num_short : a.num_rows;
    if (multi_knob == 21) a.multi_pairs = true;
    else if (multi_knob == 0) a.multi_pairs = nslots > 0 && !a.is_max && ew_heads == 1 && (double)g->E <= kMultiAvgLen * (double)nslots;
  }
  if (keep) {  // (cut after the choice above: the keeping launch runs the kernel of the filling one)
    a.num_short = (int64_t)p.num_short - p.num_empty;
    a.rider_ne = 0;
    if (a.num_short == 0 && p.num_items == 0) return TFGNN_OK;  // no edge at all: every row is an empty one
  }
  count_launch(d_out_sp ? TFGNN_KFAM_GATHER_SP : TFGNN_KFAM_GATHER);
  return gather_dispatch(a, p.num_items, (hipStream_t)stream);
}

extern "C" int tfgnn_graph_gather_reduce(const tfgnn_graph* g, int view, const int32_t* d_col_override,
                                         const float* d_edge_weight, int ew_heads, const float* d_row_scale,
                                         const float* d_in, int64_t ld_in, int width, float* d_out,
                                         int64_t ld_out, int reduce_op, int pre_act, int post_act,
                                         void* d_workspace, size_t workspace_bytes, void* stream) {
  return graph_gather_impl(g, view, d_col_override, d_edge_weight, ew_heads, d_row_scale, d_in, ld_in, width, d_out, ld_out,
                           reduce_op, pre_act, post_act, d_workspace, workspace_bytes, stream, nullptr, 0, nullptr, nullptr);
}

/* can tfgnn_graph_gather_reduce_dot take rows of `width` floats in `ew_heads` heads?  (a head = 4, 8, .. 64 floats that a
 * lane group of the gather holds in 1..16 consecutive lanes) */
extern "C" int tfgnn_graph_gather_dot_supported(int width, int ew_heads) {
  if (width <= 0 || ew_heads <= 1 || width % ew_heads) return 0;
  const int hw = width / ew_heads;
  if (hw % 4 || width % 4) return 0;
  const int lph = hw / 4, chunks = width / 4;
  if (lph & (lph - 1)) return 0;
  const int lanes_per_row = chunks <= 8 ? 8 : (chunks <= 80 ? 16 : 32);  // gather_dispatch's choice
  return lph <= 16 && lph <= lanes_per_row;
}

/* tfgnn_graph_gather_reduce with per-head edge weights that ALSO writes, per edge e of the view and head k,
 *   d_dot_out[pos(e) * ew_heads + k] = sum_{f in head k} d_in[col(e), f] * d_dot_rows[r(e) * ld_dot + f]
 * where r(e) is the row of the view the edge belongs to and pos(e) = d_dot_pos[e] (NULL: e, the edge's position in the view's
 * order).  RGAT backward: the by-source gather of d_agg[tgt] with d_dot_rows = Y yields d attention in by-target order through
 * d_dot_pos = TFGNN_G_SRC2DST_POS (replaces tfgnn_rgat_edge_dot, one pass over the edges less). */
extern "C" int tfgnn_graph_gather_reduce_dot(const tfgnn_graph* g, int view, const float* d_edge_weight, int ew_heads,
                                             const float* d_in, int64_t ld_in, int width, float* d_out, int64_t ld_out,
                                             const float* d_dot_rows, int64_t ld_dot, const int32_t* d_dot_pos, float* d_dot_out,
                                             void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(d_dot_rows && d_dot_out, "tfgnn_graph_gather_reduce_dot: NULL pointer");
  return graph_gather_impl(g, view, nullptr, d_edge_weight, ew_heads, nullptr, d_in, ld_in, width, d_out, ld_out, TFGNN_REDUCE_SUM,
                           TFGNN_ACT_NONE, TFGNN_ACT_NONE, d_workspace, workspace_bytes, stream, nullptr, 0, nullptr, nullptr, nullptr,
                           d_dot_rows, ld_dot, d_dot_pos, d_dot_out);
}

extern "C" int tfgnn_graph_gather_reduce_sp(const tfgnn_graph* g, int view, const int32_t* d_col_override,
                                            const float* d_edge_weight, const float* d_row_scale, const float* d_in,
                                            int64_t ld_in, int width, void* d_out_sp, int64_t ld_out_sp_bytes,
                                            float* d_inv_scale, const float* d_fixed_inv_scale, void* d_workspace,
                                            size_t workspace_bytes, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(d_out_sp && (d_inv_scale || d_fixed_inv_scale), "tfgnn_graph_gather_reduce_sp: NULL output");
  TFGNN_REQUIRE(ld_out_sp_bytes >= (int64_t)width * 4 && ld_out_sp_bytes % 64 == 0 && (uintptr_t)d_out_sp % 64 == 0,
                "tfgnn_graph_gather_reduce_sp: bad SP16 leading dimension / alignment");
  return graph_gather_impl(g, view, d_col_override, d_edge_weight, 1, d_row_scale, d_in, ld_in, width, nullptr, 0,
                           TFGNN_REDUCE_SUM, TFGNN_ACT_NONE, TFGNN_ACT_NONE, d_workspace, workspace_bytes, stream, d_out_sp,
                           ld_out_sp_bytes, d_inv_scale, d_fixed_inv_scale);
}

/* tfgnn_graph_gather_reduce_sp into an operand that already holds the rows and marker scales of the view's empty buckets
 * (keep_empty_rows != 0; the contract is stated in include/tfgnn.h): they are neither read nor written. */
extern "C" int tfgnn_graph_gather_reduce_sp_keep_empty(const tfgnn_graph* g, int view, const int32_t* d_col_override,
                                                       const float* d_edge_weight, const float* d_row_scale, const float* d_in,
                                                       int64_t ld_in, int width, void* d_out_sp, int64_t ld_out_sp_bytes,
                                                       float* d_inv_scale, const float* d_fixed_inv_scale, void* d_workspace,
                                                       size_t workspace_bytes, int keep_empty_rows, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(d_out_sp && (d_inv_scale || d_fixed_inv_scale), "tfgnn_graph_gather_reduce_sp_keep_empty: NULL output");
  TFGNN_REQUIRE(ld_out_sp_bytes >= (int64_t)width * 4 && ld_out_sp_bytes % 64 == 0 && (uintptr_t)d_out_sp % 64 == 0,
                "tfgnn_graph_gather_reduce_sp_keep_empty: bad SP16 leading dimension / alignment");
  return graph_gather_impl(g, view, d_col_override, d_edge_weight, 1, d_row_scale, d_in, ld_in, width, nullptr, 0,
                           TFGNN_REDUCE_SUM, TFGNN_ACT_NONE, TFGNN_ACT_NONE, d_workspace, workspace_bytes, stream, d_out_sp,
                           ld_out_sp_bytes, d_inv_scale, d_fixed_inv_scale, nullptr, nullptr, 0, nullptr, nullptr,
                           keep_empty_rows != 0);
}

/* tfgnn_graph_gather_reduce_sp in the form that used to hand the combine pass of the long buckets back as a job for
 * tfgnn_aux_launch: the gather combines them in its own launch now, *combine_job always comes back empty (kind 0). */
extern "C" int tfgnn_graph_gather_reduce_sp_deferred(const tfgnn_graph* g, int view, const int32_t* d_col_override,
                                                     const float* d_edge_weight, const float* d_row_scale, const float* d_in,
                                                     int64_t ld_in, int width, void* d_out_sp, int64_t ld_out_sp_bytes,
                                                     float* d_inv_scale, const float* d_fixed_inv_scale, void* d_workspace,
                                                     size_t workspace_bytes, tfgnn_aux_job* combine_job, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(d_out_sp && (d_inv_scale || d_fixed_inv_scale) && combine_job, "tfgnn_graph_gather_reduce_sp_deferred: NULL output");
  TFGNN_REQUIRE(ld_out_sp_bytes >= (int64_t)width * 4 && ld_out_sp_bytes % 64 == 0 && (uintptr_t)d_out_sp % 64 == 0,
                "tfgnn_graph_gather_reduce_sp_deferred: bad SP16 leading dimension / alignment");
  return graph_gather_impl(g, view, d_col_override, d_edge_weight, 1, d_row_scale, d_in, ld_in, width, nullptr, 0,
                           TFGNN_REDUCE_SUM, TFGNN_ACT_NONE, TFGNN_ACT_NONE, d_workspace, workspace_bytes, stream, d_out_sp,
                           ld_out_sp_bytes, d_inv_scale, d_fixed_inv_scale, combine_job);
}
