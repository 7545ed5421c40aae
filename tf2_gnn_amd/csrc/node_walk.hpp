// The skeleton the walks of basis.hip and blockdiag.hip share over a NODE view of the graph handle (all edge types of a node in
// one row, the edges of a row sorted by type) and that view's long-row plan (graph.hpp CsrPlan):
//   * one launch does both kinds of work.  Workgroups [0, num_items) take one item of a long row each (item_chunk_edges edges):
//     the 256 / LPR lane groups take consecutive slices of the item's edges, their sums meet in LDS and are added in group
//     order.  The other workgroups take 256 / LPR short rows each, one lane group per row, and leave alone the rows longer
//     than long_threshold;
//   * an item that is its whole row (item_slot < 0) writes the output row itself, times the node scale.  A row made of several
//     items leaves one unscaled partial row per item in the workspace, and a second, small launch (node_walk.hip) adds them in
//     item order and applies the node scale.  Nobody counts arrivals or waits for another workgroup.
// What a lane group does with its edges, and which output column an LDS entry belongs to, is the caller's.
// blockdiag.hip's walk kernel keeps its own copy of the range and of the epilogue, and its argument struct its own field order:
// routed through group_range and with the plan fields first, two of its per-call timings at D = H = 320 moved beyond the
// parent's run-to-run spread (NOTEBOOK 49).  It shares the rest: Vec, fill_plan, the dispatch, the launches, the host checks.
// Not for spmm.hip and rgat.hip: their long rows finish inside the kernel (arrival counters, two-phase softmax items).
#pragma once
#include <atomic>
#include <type_traits>

#include "common.hpp"
#include "graph.hpp"

namespace tfgnn {

template <int VEC>
struct Vec {
  float v[VEC];
};
template <int VEC>
__device__ __forceinline__ Vec<VEC> load_vec(const float* p, bool live) {
  Vec<VEC> r;
  if constexpr (VEC == 4) {
    const float4 t = live ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = live ? *p : 0.f;
  }
  return r;
}
template <int VEC>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[VEC], float scale) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale);
  else *p = v[0] * scale;
}

// what every walk's kernel argument starts with
struct NodeWalkArgs {
  const int32_t* nodeptr;  // [V+1] the node view's row pointers
  const int32_t* coll;     // [E]   other end * L + type
  int64_t V;
  int L;
  const float* ew;  // [E] in the view's edge order, or NULL (= 1)
  const float* ns;  // [V] m_v, or NULL (= 1)
  float* partial;   // [num_partials, row width]
  int long_threshold, item_chunk_edges, num_items;
  const int32_t *item_row, *item_chunk, *item_slot;
};

// Args: NodeWalkArgs, or a struct that carries the same fields under the same names in an order of its own
template <class Args>
void fill_plan(Args& a, const GraphView& gv) {
  const CsrPlan& p = gv.plan;
  a.nodeptr = gv.rowptr; a.coll = gv.col;
  a.long_threshold = p.long_threshold; a.item_chunk_edges = p.item_chunk_edges; a.num_items = p.num_items;
  a.item_row = p.item_row; a.item_chunk = p.item_chunk; a.item_slot = p.item_slot;
}

// The edges [beg, end) lane group `group` of workgroup `bx` walks.  whole_row: they are short row `row`, or, with row < 0,
// nothing: the row is past V, or a long row, which the item workgroups take.  Otherwise they are a slice (possibly empty) of
// item `item` of row `row`, and every lane group of the workgroup goes on to item_epilogue.  whole_row is the same for the whole
// workgroup; it is a field of its own so that the caller's test folds into the one made here.
struct GroupRange {
  bool whole_row;
  int64_t row;
  int32_t beg, end;
  int item;
};
template <int GROUPS>
__device__ __forceinline__ GroupRange group_range(const NodeWalkArgs& a, int bx, int group) {
  GroupRange r;
  r.whole_row = bx >= a.num_items;
  r.item = bx;
  if (r.whole_row) {  // short rows, in node order
    r.row = ((int64_t)bx - a.num_items) * GROUPS + group;
    r.beg = r.end = 0;
    if (r.row >= a.V) {
      r.row = -1;
      return r;
    }
    r.beg = a.nodeptr[r.row];
    r.end = a.nodeptr[r.row + 1];
    if (r.end - r.beg > a.long_threshold) r.row = -1;
    return r;
  }
  r.row = a.item_row[bx];
  const int32_t rbeg = a.nodeptr[r.row], rend = a.nodeptr[r.row + 1];
  const int32_t ibeg = min(rend, rbeg + a.item_chunk[bx] * a.item_chunk_edges);
  const int32_t iend = min(rend, ibeg + a.item_chunk_edges);
  const int per = (iend - ibeg + GROUPS - 1) / GROUPS;  // consecutive edges per lane group
  r.beg = min(iend, ibeg + group * per);
  r.end = min(iend, r.beg + per);
  return r;
}

// The end of an item workgroup (all 256 threads): lane (group, gl) leaves acc[j][c] at red[group][j * LPR * VEC + gl * VEC + c],
// then entry f < n is the groups' entries added in group order and goes to column col(f) (a Column; not valid: no such column)
// of the row's own output, times ns[row], when the item is the whole row, of the item's partial row, unscaled, otherwise.
template <class T>
struct Column {
  bool valid;
  T col;
};
template <int VEC, int LPR, int NACC, class Col>
__device__ __forceinline__ void item_epilogue(const NodeWalkArgs& a, const GroupRange& r, float (&red)[256 / LPR][NACC * LPR * VEC],
                                              const float (&acc)[NACC][VEC], const float* ns, float* out, int64_t ld_out, int width,
                                              int n, Col col) {
  constexpr int GROUPS = 256 / LPR, PW = LPR * VEC;
  const int tid = threadIdx.x, group = tid / LPR, gl = tid % LPR;
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int c = 0; c < VEC; ++c) red[group][j * PW + gl * VEC + c] = acc[j][c];
  __syncthreads();
  const int32_t slot = a.item_slot[r.item];
  const float m = (ns && slot < 0) ? ns[r.row] : 1.f;
  float* orow = slot < 0 ? out + r.row * ld_out : a.partial + (int64_t)slot * width;
  for (int f = tid; f < n; f += 256) {
    const auto o = col(f);
    if (!o.valid) continue;
    float s = red[0][f];
#pragma unroll
    for (int g = 1; g < GROUPS; ++g) s += red[g][f];
    orow[o.col] = s * m;
  }
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
inline bool rows_aligned(const void* p, int64_t ld) { return (uintptr_t)p % 16 == 0 && ld % 4 == 0; }

// what every entry asks of its graph handle, before anything touches the device; `who` names the entry in the message
inline int check_graph(const char* who, const tfgnn_graph* g) {
  TFGNN_REQUIRE(g != nullptr, "%s: graph is NULL", who);
  TFGNN_REQUIRE(g->L >= 1 && g->L <= 256, "%s: %d edge types, the graph handle's limit is 1 <= L <= 256", who, g->L);
  return graph_require_parts(g, TFGNN_GRAPH_PART_PLAN_NODE, who);
}

// f(VEC, LPR) as std::integral_constants: vector path (4 floats per lane) or scalar, lane groups of 16, 32 or 64 lanes
template <class F>
void dispatch_shape(bool vec, int lpr, F&& f) {
  using std::integral_constant;
  if (vec) {
    if (lpr == 16) f(integral_constant<int, 4>{}, integral_constant<int, 16>{});
    else if (lpr == 32) f(integral_constant<int, 4>{}, integral_constant<int, 32>{});
    else f(integral_constant<int, 4>{}, integral_constant<int, 64>{});
  } else {
    if (lpr == 16) f(integral_constant<int, 1>{}, integral_constant<int, 16>{});
    else if (lpr == 32) f(integral_constant<int, 1>{}, integral_constant<int, 32>{});
    else f(integral_constant<int, 1>{}, integral_constant<int, 64>{});
  }
}

// rows made of several items: out[row, :] = ns[row] * (the row's partial rows added in item order); node_walk.hip
int node_walk_combine(const CsrPlan& p, const float* partial, int width, const float* ns, float* out, int64_t ld_out, hipStream_t s);

// walk() launches the walk kernel; then, when some row has several items, the launch that adds their partial rows.  Every
// launch is counted on `counter`.  `ns`: the node scale the walk kernel hands to item_epilogue (the combine applies the same).
template <class Walk>
int launch_walk(Walk&& walk, const GraphView& gv, const float* partial, const float* ns, int width, float* out, int64_t ld_out,
                std::atomic<int64_t>& counter, hipStream_t s) {
  walk();
  TFGNN_LAUNCH_CHECK();
  counter.fetch_add(1, std::memory_order_relaxed);
  if (gv.plan.num_multi > 0) {
    const int rc = node_walk_combine(gv.plan, partial, width, ns, out, ld_out, s);
    if (rc) return rc;
    counter.fetch_add(1, std::memory_order_relaxed);
  }
  return TFGNN_OK;
}

}  // namespace tfgnn
