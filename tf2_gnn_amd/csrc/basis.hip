// R-GCN basis decomposition (Schlichtkrull et al., eq. 3: W_l = sum_b a[l,b] V_b), aggregate first:
//   Z[v, b, :] = m_v * sum_{e = (u -> v), type l} s_e * a[l,b] * X[u, :]          tfgnn_basis_gather_forward
//   out        = act(Z.reshape(V, B*D) @ [V_0; ...; V_{B-1}])                      (the existing products)
// and the two reverse passes of the gather (tfgnn_basis_gather_backward).  The contracts and the order of every sum are
// stated in include/tfgnn.h ("R-GCN basis decomposition"); DESIGN.md has the byte model.
//
// All three walks share one skeleton over a NODE view of the graph handle (all edge types of a node in one row, the edges of
// a row sorted by type) and that view's long-row plan (graph.hpp CsrPlan):
//   * a row of at most long_threshold edges is walked by one lane group (LPR lanes over the feature columns, VEC floats each);
//   * a longer row is cut into items of item_chunk_edges edges, one workgroup per item: the 256 / LPR lane groups take
//     consecutive runs of the item's edges, their sums meet in LDS and are added in group order;
//   * a row made of several items leaves one partial row per item in the workspace, and a second, small launch adds them
//     in item order.  Nobody counts arrivals or waits for another workgroup.
// blockIdx.y walks the feature windows (LPR * VEC columns) and, in the forward and coefficient walks, the tiles of bases.
#include <atomic>

#include "common.hpp"
#include "graph.hpp"

namespace tfgnn {
namespace {

constexpr int FWD_BT = 8;      // bases a lane accumulates at once in the forward walk (FWD_BT * VEC registers)
constexpr int DC_BT = 16;      // bases per tile of the coefficient walk (one dot product each)
constexpr int RED_NODES = 1024;  // nodes per workgroup of the coefficient reduction's first stage
constexpr int MAX_D = 1 << 20;

std::atomic<int64_t> g_basis_launches[3];  // forward, dX, dcoeff

struct BasisArgs {
  const int32_t* nodeptr;  // [V+1] the node view's row pointers
  const int32_t* coll;     // [E]   other end * L + type
  int64_t V;
  int L, B, D;
  const float* coeff;  // [L, B]
  const float* ew;     // [E] in the view's edge order, or NULL (= 1)
  const float* ns;     // [V] m_v, or NULL (= 1)
  const float* in;     // forward, dcoeff: X [V, D]; dX: dZ [V, B*D]
  int64_t ld_in;
  const float* dz;  // dcoeff: dZ
  int64_t ld_dz;
  float* out;  // forward: Z; dX: dX; dcoeff: P [E, B] (dot products at the first edge of every run)
  int64_t ld_out;
  float* partial;  // [num_partials, row width]
  int long_threshold, item_chunk_edges, num_items;
  const int32_t *item_row, *item_chunk, *item_slot;
};

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

// ---- forward: edges [beg, end) of target row -> acc[j][:] = sum over the type runs (ascending) of a[l, b0+j] * run sum, the
// run sum taken over the run's edges in order: run = fma(s_e, x, run) ----
template <int VEC>
__device__ __forceinline__ void forward_walk(const BasisArgs& a, int32_t beg, int32_t end, int d, bool live, int b0,
                                             float (&acc)[FWD_BT][VEC]) {
  float run[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) run[c] = 0.f;
  int cur = -1;
  auto fold = [&](int l) {
#pragma unroll
    for (int j = 0; j < FWD_BT; ++j) {
      if (b0 + j < a.B) {
        const float cf = a.coeff[(int64_t)l * a.B + b0 + j];
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc[j][c] = fmaf(cf, run[c], acc[j][c]);
      }
    }
  };
  for (int32_t e = beg; e < end; e += 4) {  // four source rows in flight
    int32_t cl[4];
    float w[4];
    Vec<VEC> x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int32_t ee = min(e + u, end - 1);
      cl[u] = a.coll[ee];
      w[u] = a.ew ? a.ew[ee] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = load_vec<VEC>(a.in + (int64_t)(cl[u] / a.L) * a.ld_in + d, live);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (e + u < end) {
        const int t = cl[u] % a.L;
        if (t != cur) {
          if (cur >= 0) fold(cur);
          cur = t;
#pragma unroll
          for (int c = 0; c < VEC; ++c) run[c] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < VEC; ++c) run[c] = fmaf(w[u], x[u].v[c], run[c]);
      }
    }
  }
  if (cur >= 0) fold(cur);
}

// ---- dX: edges [beg, end) of a source row -> acc += s'_e * (sum over b ascending of a[l,b] * dZ[v, b, :]) in edge order ----
template <int VEC>
__device__ __forceinline__ void dx_walk(const BasisArgs& a, int32_t beg, int32_t end, int d, bool live, float (&acc)[VEC]) {
  for (int32_t e = beg; e < end; ++e) {
    const int32_t cl = a.coll[e];
    const int v = cl / a.L, l = cl - v * a.L;
    const float w = a.ew ? a.ew[e] : 1.f;
    const float* zrow = a.in + (int64_t)v * a.ld_in + d;
    const float* cf = a.coeff + (int64_t)l * a.B;
    float t[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) t[c] = 0.f;
#pragma unroll 4
    for (int b = 0; b < a.B; ++b) {
      const Vec<VEC> z = load_vec<VEC>(zrow + (int64_t)b * a.D, live);
      const float k = cf[b];
#pragma unroll
      for (int c = 0; c < VEC; ++c) t[c] = fmaf(k, z.v[c], t[c]);
    }
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[c] = fmaf(w, t[c], acc[c]);
  }
}

// One launch, both kinds of work: workgroups [0, num_items) take one item of a long row each, the others 256 / LPR short rows.
// FWD: NACC = FWD_BT accumulators per lane (bases b0 ..), output column (b0 + j) * D + d; otherwise one, output column d.
template <int VEC, int LPR, bool FWD>
__global__ void __launch_bounds__(256) basis_rows_kernel(BasisArgs a) {
  constexpr int GROUPS = 256 / LPR;
  constexpr int PW = LPR * VEC;  // feature window
  constexpr int NACC = FWD ? FWD_BT : 1;
  __shared__ float red[GROUPS][NACC * PW];
  const int tid = threadIdx.x, group = tid / LPR, gl = tid % LPR;
  const int windows = (a.D + PW - 1) / PW;
  const int win = blockIdx.y % windows;
  const int b0 = FWD ? (int)(blockIdx.y / windows) * FWD_BT : 0;
  const int d = win * PW + gl * VEC;
  const bool live = d < a.D;
  const int width = FWD ? a.B * a.D : a.D;  // floats per output row
  float acc[NACC][VEC];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[j][c] = 0.f;

  if ((int)blockIdx.x >= a.num_items) {  // short rows, in node order: one lane group per row, no LDS
    const int64_t row = ((int64_t)blockIdx.x - a.num_items) * GROUPS + group;
    if (row >= a.V) return;
    const int32_t beg = a.nodeptr[row], end = a.nodeptr[row + 1];
    if (end - beg > a.long_threshold || !live) return;  // long rows: the item workgroups
    if constexpr (FWD) forward_walk<VEC>(a, beg, end, d, live, b0, acc);
    else dx_walk<VEC>(a, beg, end, d, live, acc[0]);
    const float m = (FWD && a.ns) ? a.ns[row] : 1.f;
    float* orow = a.out + row * a.ld_out;
#pragma unroll
    for (int j = 0; j < NACC; ++j)
      if (!FWD || b0 + j < a.B) store_vec<VEC>(orow + (int64_t)(b0 + j) * a.D + d, acc[j], m);
    return;
  }

  const int item = blockIdx.x;
  const int64_t row = a.item_row[item];
  const int32_t rbeg = a.nodeptr[row], rend = a.nodeptr[row + 1];
  const int32_t ibeg = min(rend, rbeg + a.item_chunk[item] * a.item_chunk_edges);
  const int32_t iend = min(rend, ibeg + a.item_chunk_edges);
  const int per = (iend - ibeg + GROUPS - 1) / GROUPS;  // consecutive edges per lane group
  const int32_t beg = min(iend, ibeg + group * per), end = min(iend, beg + per);
  if (live) {
    if constexpr (FWD) forward_walk<VEC>(a, beg, end, d, live, b0, acc);
    else dx_walk<VEC>(a, beg, end, d, live, acc[0]);
  }
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int c = 0; c < VEC; ++c) red[group][j * PW + gl * VEC + c] = acc[j][c];
  __syncthreads();
  const int32_t slot = a.item_slot[item];
  const float m = (FWD && a.ns && slot < 0) ? a.ns[row] : 1.f;
  float* orow = slot < 0 ? a.out + row * a.ld_out : a.partial + (int64_t)slot * width;
  for (int f = tid; f < NACC * PW; f += 256) {
    const int j = f / PW, dd = win * PW + f % PW;
    if (dd >= a.D || (FWD && b0 + j >= a.B)) continue;
    float s = red[0][f];
#pragma unroll
    for (int g = 1; g < GROUPS; ++g) s += red[g][f];
    orow[(int64_t)(b0 + j) * a.D + dd] = s * m;
  }
}

// rows made of several items: out[row, :] = m_row * (partial rows of the row added in item order)
__global__ void __launch_bounds__(256)
basis_combine_kernel(const int32_t* __restrict__ multi_row, const int32_t* __restrict__ multi_base, const int32_t* __restrict__ multi_n,
                     const float* __restrict__ partial, int width, const float* __restrict__ ns, float* __restrict__ out,
                     int64_t ld_out) {
  const int m = blockIdx.x;
  const int64_t row = multi_row[m];
  const int32_t base = multi_base[m], n = multi_n[m];
  const float scale = ns ? ns[row] : 1.f;
  for (int f = blockIdx.y * 256 + threadIdx.x; f < width; f += gridDim.y * 256) {
    float s = partial[(int64_t)base * width + f];
    for (int k = 1; k < n; ++k) s += partial[(int64_t)(base + k) * width + f];
    out[row * ld_out + f] = s * scale;
  }
}

// ---- dcoeff, walk: for every run of one edge type inside the edges a lane group walks, P[first edge of the run, b] =
// m_v * <run sum of s_e X[u_e, :], dZ[v, b, :]>.  The run sum is never stored.  blockIdx.y: tile of DC_BT bases. ----
template <int VEC, int LPR>
__global__ void __launch_bounds__(256) basis_dcoeff_walk_kernel(BasisArgs a) {
  constexpr int GROUPS = 256 / LPR;
  constexpr int PW = LPR * VEC;
  const int tid = threadIdx.x, group = tid / LPR, gl = tid % LPR;
  const int b0 = blockIdx.y * DC_BT;
  int64_t row;
  int32_t beg, end;
  if ((int)blockIdx.x >= a.num_items) {
    row = ((int64_t)blockIdx.x - a.num_items) * GROUPS + group;
    if (row >= a.V) return;
    beg = a.nodeptr[row];
    end = a.nodeptr[row + 1];
    if (end - beg > a.long_threshold) return;
  } else {
    const int item = blockIdx.x;
    row = a.item_row[item];
    const int32_t rbeg = a.nodeptr[row], rend = a.nodeptr[row + 1];
    const int32_t ibeg = min(rend, rbeg + a.item_chunk[item] * a.item_chunk_edges);
    const int32_t iend = min(rend, ibeg + a.item_chunk_edges);
    const int per = (iend - ibeg + GROUPS - 1) / GROUPS;
    beg = min(iend, ibeg + group * per);
    end = min(iend, beg + per);
  }
  const float m = a.ns ? a.ns[row] : 1.f;
  const float* zrow = a.dz + row * a.ld_dz;
  // every lane of the group runs the same loops (the shuffles below stay inside the group)
  int32_t e = beg;
  while (e < end) {
    const int l = a.coll[e] % a.L;
    int32_t e1 = e + 1;
    while (e1 < end && a.coll[e1] % a.L == l) ++e1;
    float dot[DC_BT];
#pragma unroll
    for (int j = 0; j < DC_BT; ++j) dot[j] = 0.f;
    for (int d0 = 0; d0 < a.D; d0 += PW) {
      const int d = d0 + gl * VEC;
      const bool live = d < a.D;
      float run[VEC];
#pragma unroll
      for (int c = 0; c < VEC; ++c) run[c] = 0.f;
      for (int32_t ee = e; ee < e1; ++ee) {
        const Vec<VEC> x = load_vec<VEC>(a.in + (int64_t)(a.coll[ee] / a.L) * a.ld_in + d, live);
        const float w = a.ew ? a.ew[ee] : 1.f;
#pragma unroll
        for (int c = 0; c < VEC; ++c) run[c] = fmaf(w, x.v[c], run[c]);
      }
#pragma unroll
      for (int j = 0; j < DC_BT; ++j) {
        if (b0 + j < a.B) {
          const Vec<VEC> z = load_vec<VEC>(zrow + (int64_t)(b0 + j) * a.D + d, live);
#pragma unroll
          for (int c = 0; c < VEC; ++c) dot[j] = fmaf(run[c], z.v[c], dot[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < DC_BT; ++j)
#pragma unroll
      for (int o = LPR / 2; o; o >>= 1) dot[j] += __shfl_xor(dot[j], o, LPR);
    if (gl == 0) {
#pragma unroll
      for (int j = 0; j < DC_BT; ++j)
        if (b0 + j < a.B) a.out[(int64_t)e * a.B + b0 + j] = dot[j] * m;
    }
    e = e1;
  }
}

// ---- dcoeff, reduction stage 1: workgroup (chunk c of RED_NODES nodes, type l), lane = basis.  Wave w adds the P rows of the
// edges of bucket (v, l) in edge order for v = c * RED_NODES + w, + 4, ...; the four waves' sums are added in wave order. ----
__global__ void __launch_bounds__(256)
basis_dcoeff_reduce1_kernel(const int32_t* __restrict__ rowptr_typed, const float* __restrict__ P, int64_t V, int L, int B,
                            float* __restrict__ part2) {
  __shared__ float red[4][64];
  const int c = blockIdx.x, l = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t v1 = min(V, (int64_t)(c + 1) * RED_NODES);
  float acc = 0.f;
  for (int64_t v = (int64_t)c * RED_NODES + wave; v < v1; v += 4) {
    const int32_t e0 = rowptr_typed[v * L + l], e1 = rowptr_typed[v * L + l + 1];
    if (lane < B)
      for (int32_t e = e0; e < e1; ++e) acc += P[(int64_t)e * B + lane];
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (threadIdx.x < B)
    part2[((int64_t)l * gridDim.x + c) * B + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// stage 2: dcoeff[l, b] = the chunk sums in chunk order
__global__ void __launch_bounds__(256)
basis_dcoeff_reduce2_kernel(const float* __restrict__ part2, int chunks, int LB, int B, float* __restrict__ dcoeff) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= LB) return;
  const int l = i / B, b = i - l * B;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part2[((int64_t)l * chunks + c) * B + b];
  dcoeff[i] = s;
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
inline int64_t red_chunks(int64_t V) { return std::max<int64_t>(1, ceil_div(V, RED_NODES)); }

struct Shape {
  bool vec;
  int lpr;
};
// vector path: D % 4 == 0 and every row 16-byte aligned; the lane group is as wide as the row needs (16, 32 or 64 lanes)
inline Shape pick_shape(int D, bool aligned) {
  Shape s;
  s.vec = D % 4 == 0 && aligned;
  const int chunks = s.vec ? D / 4 : D;
  s.lpr = chunks <= 16 ? 16 : (chunks <= 32 && s.vec ? 32 : 64);
  return s;
}
inline bool rows_aligned(const void* p, int64_t ld) { return (uintptr_t)p % 16 == 0 && ld % 4 == 0; }

template <bool FWD>
void launch_rows(const Shape& sh, const BasisArgs& a, dim3 grid, hipStream_t s) {
  if (sh.vec) {
    if (sh.lpr == 16) hipLaunchKernelGGL((basis_rows_kernel<4, 16, FWD>), grid, dim3(256), 0, s, a);
    else if (sh.lpr == 32) hipLaunchKernelGGL((basis_rows_kernel<4, 32, FWD>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((basis_rows_kernel<4, 64, FWD>), grid, dim3(256), 0, s, a);
  } else {
    if (sh.lpr == 16) hipLaunchKernelGGL((basis_rows_kernel<1, 16, FWD>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((basis_rows_kernel<1, 64, FWD>), grid, dim3(256), 0, s, a);
  }
}
void launch_dcoeff_walk(const Shape& sh, const BasisArgs& a, dim3 grid, hipStream_t s) {
  if (sh.vec) {
    if (sh.lpr == 16) hipLaunchKernelGGL((basis_dcoeff_walk_kernel<4, 16>), grid, dim3(256), 0, s, a);
    else if (sh.lpr == 32) hipLaunchKernelGGL((basis_dcoeff_walk_kernel<4, 32>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((basis_dcoeff_walk_kernel<4, 64>), grid, dim3(256), 0, s, a);
  } else {
    if (sh.lpr == 16) hipLaunchKernelGGL((basis_dcoeff_walk_kernel<1, 16>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((basis_dcoeff_walk_kernel<1, 64>), grid, dim3(256), 0, s, a);
  }
}

// the checks both entries share, before anything touches the device; `who` names the entry in the message
int check_limits(const char* who, const tfgnn_graph* g, int B, int D) {
  if (B < 1 || B > 64) {
    set_error("%s: num_bases = %d is outside the limit 1 <= num_bases <= 64", who, B);
    return B > 64 ? TFGNN_ERR_UNSUPPORTED : TFGNN_ERR_INVALID_ARGUMENT;
  }
  TFGNN_REQUIRE(D >= 1, "%s: D = %d, the limit is D >= 1", who, D);
  if (D > MAX_D) {
    set_error("%s: D = %d is above the limit D <= %d", who, D, MAX_D);
    return TFGNN_ERR_UNSUPPORTED;
  }
  TFGNN_REQUIRE(g != nullptr, "%s: graph is NULL", who);
  TFGNN_REQUIRE(g->L >= 1 && g->L <= 256, "%s: %d edge types, the graph handle's limit is 1 <= L <= 256", who, g->L);
  return graph_require_parts(g, TFGNN_GRAPH_PART_PLAN_NODE, who);
}

void fill_plan(BasisArgs& a, const GraphView& gv) {
  const CsrPlan& p = gv.plan;
  a.nodeptr = gv.rowptr; a.coll = gv.col;
  a.long_threshold = p.long_threshold; a.item_chunk_edges = p.item_chunk_edges; a.num_items = p.num_items;
  a.item_row = p.item_row; a.item_chunk = p.item_chunk; a.item_slot = p.item_slot;
}

}  // namespace
}  // namespace tfgnn

extern "C" size_t tfgnn_basis_workspace_bytes(int64_t V, int64_t E, int L, int B, int D, int64_t partials_by_dst,
                                              int64_t partials_by_src) {
  using namespace tfgnn;
  if (V < 0 || E < 0 || L < 1 || B < 1 || B > 64 || D < 1 || partials_by_dst < 0 || partials_by_src < 0) return 0;
  const size_t fwd = align16((size_t)partials_by_dst * B * D * 4);
  const size_t bwd = align16((size_t)partials_by_src * D * 4) + align16((size_t)E * B * 4) + align16((size_t)L * red_chunks(V) * B * 4);
  return std::max(fwd, bwd);
}

extern "C" int tfgnn_basis_launch_counts(int64_t* out_counts, int n) {
  using namespace tfgnn;
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_basis_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i < 3 ? g_basis_launches[i].load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

extern "C" int tfgnn_basis_gather_forward(const tfgnn_basis_forward_args* p, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(p != nullptr && p->struct_size == sizeof(tfgnn_basis_forward_args),
                "tfgnn_basis_gather_forward: args is NULL or was built against another header (struct_size)");
  const int rc = check_limits("tfgnn_basis_gather_forward", p->graph, p->B, p->D);
  if (rc) return rc;
  const tfgnn_graph* g = p->graph;
  const int B = p->B, D = p->D;
  const int64_t width = (int64_t)B * D;
  TFGNN_REQUIRE(width < ((int64_t)1 << 31), "tfgnn_basis_gather_forward: B * D = %lld, the limit is B * D < 2^31", (long long)width);
  if (g->V == 0) return TFGNN_OK;
  TFGNN_REQUIRE(p->coeff && p->X && p->Z, "tfgnn_basis_gather_forward: NULL pointer");
  TFGNN_REQUIRE(p->ldX >= D && p->ldZ >= width, "tfgnn_basis_gather_forward: a row stride is smaller than its row");
  const GraphView& gv = g->views[1];  // by target, all edge types of a node in one row
  const size_t need = (size_t)gv.plan.num_partials * width * 4;
  TFGNN_REQUIRE(need == 0 || (p->workspace && p->workspace_bytes >= need && (uintptr_t)p->workspace % 16 == 0),
                "tfgnn_basis_gather_forward: workspace too small or not 16-byte aligned: need %zu bytes", need);
  BasisArgs a{};
  fill_plan(a, gv);
  a.V = g->V; a.L = g->L; a.B = B; a.D = D; a.coeff = p->coeff; a.ew = p->edge_weight_by_dst; a.ns = p->node_scale;
  a.in = p->X; a.ld_in = p->ldX; a.out = p->Z; a.ld_out = p->ldZ; a.partial = (float*)p->workspace;
  const Shape sh = pick_shape(D, rows_aligned(p->X, p->ldX) && rows_aligned(p->Z, p->ldZ));
  const int pw = sh.lpr * (sh.vec ? 4 : 1);
  const int64_t gy = ceil_div(D, pw) * ceil_div(B, FWD_BT);
  TFGNN_REQUIRE(gy <= 65535, "tfgnn_basis_gather_forward: D = %d with B = %d needs more than 65535 feature windows", D, B);
  const int64_t gx = a.num_items + ceil_div(g->V, 256 / sh.lpr);
  hipStream_t s = (hipStream_t)stream;
  launch_rows<true>(sh, a, dim3((unsigned)gx, (unsigned)gy), s);
  TFGNN_LAUNCH_CHECK();
  g_basis_launches[0].fetch_add(1, std::memory_order_relaxed);
  if (gv.plan.num_multi > 0) {
    hipLaunchKernelGGL(basis_combine_kernel, dim3((unsigned)gv.plan.num_multi, (unsigned)std::min<int64_t>(ceil_div(width, 256), 64)),
                       dim3(256), 0, s, gv.plan.multi_row, gv.plan.multi_base, gv.plan.multi_n, a.partial, (int)width, a.ns, a.out,
                       a.ld_out);
    TFGNN_LAUNCH_CHECK();
    g_basis_launches[0].fetch_add(1, std::memory_order_relaxed);
  }
  return TFGNN_OK;
}

extern "C" int tfgnn_basis_gather_backward(const tfgnn_basis_backward_args* p, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(p != nullptr && p->struct_size == sizeof(tfgnn_basis_backward_args),
                "tfgnn_basis_gather_backward: args is NULL or was built against another header (struct_size)");
  const int rc = check_limits("tfgnn_basis_gather_backward", p->graph, p->B, p->D);
  if (rc) return rc;
  const tfgnn_graph* g = p->graph;
  const int B = p->B, D = p->D, L = g->L;
  const int64_t width = (int64_t)B * D, V = g->V, E = g->E;
  TFGNN_REQUIRE(width < ((int64_t)1 << 31), "tfgnn_basis_gather_backward: B * D = %lld, the limit is B * D < 2^31", (long long)width);
  if (!p->dX && !p->dcoeff) return TFGNN_OK;
  hipStream_t s = (hipStream_t)stream;
  TFGNN_REQUIRE(V == 0 || (p->coeff && p->dZ && p->lddZ >= width), "tfgnn_basis_gather_backward: dZ / coeff NULL or dZ's row stride too small");
  TFGNN_REQUIRE(!p->dX || V == 0 || p->lddX >= D, "tfgnn_basis_gather_backward: dX's row stride is smaller than D");
  TFGNN_REQUIRE(!p->dcoeff || V == 0 || (p->X && p->ldX >= D), "tfgnn_basis_gather_backward: dcoeff needs X with a row stride >= D");
  const GraphView& gs = g->views[3];  // by source
  const GraphView& gd = g->views[1];  // by target
  const int64_t chunks = red_chunks(V);
  const size_t o_P = align16((size_t)gs.plan.num_partials * D * 4);
  const size_t o_part2 = o_P + align16((size_t)E * B * 4);
  const size_t need = o_part2 + align16((size_t)L * chunks * B * 4);
  TFGNN_REQUIRE(V == 0 || (p->workspace && p->workspace_bytes >= need && (uintptr_t)p->workspace % 16 == 0),
                "tfgnn_basis_gather_backward: workspace too small or not 16-byte aligned: need %zu bytes", need);
  const int64_t gy_dc = ceil_div(B, DC_BT);
  char* ws = (char*)p->workspace;

  if (p->dX && V > 0) {
    BasisArgs a{};
    fill_plan(a, gs);
    a.V = V; a.L = L; a.B = B; a.D = D; a.coeff = p->coeff; a.ew = p->edge_weight_by_src;
    a.in = p->dZ; a.ld_in = p->lddZ; a.out = p->dX; a.ld_out = p->lddX; a.partial = (float*)ws;
    const Shape sh = pick_shape(D, rows_aligned(p->dZ, p->lddZ) && rows_aligned(p->dX, p->lddX));
    const int pw = sh.lpr * (sh.vec ? 4 : 1);
    launch_rows<false>(sh, a, dim3((unsigned)(a.num_items + ceil_div(V, 256 / sh.lpr)), (unsigned)ceil_div(D, pw)), s);
    TFGNN_LAUNCH_CHECK();
    g_basis_launches[1].fetch_add(1, std::memory_order_relaxed);
    if (gs.plan.num_multi > 0) {
      hipLaunchKernelGGL(basis_combine_kernel, dim3((unsigned)gs.plan.num_multi, (unsigned)std::min<int64_t>(ceil_div(D, 256), 64)), dim3(256), 0,
                         s, gs.plan.multi_row, gs.plan.multi_base, gs.plan.multi_n, a.partial, D, (const float*)nullptr, a.out, a.ld_out);
      TFGNN_LAUNCH_CHECK();
      g_basis_launches[1].fetch_add(1, std::memory_order_relaxed);
    }
  }
  if (p->dcoeff) {
    if (V == 0 || E == 0) {  // no edge, no term: zeros
      TFGNN_HIP_CHECK(hipMemsetAsync(p->dcoeff, 0, (size_t)L * B * 4, s));
      return TFGNN_OK;
    }
    float* P = (float*)(ws + o_P);
    float* part2 = (float*)(ws + o_part2);
    TFGNN_HIP_CHECK(hipMemsetAsync(P, 0, (size_t)E * B * 4, s));
    BasisArgs a{};
    fill_plan(a, gd);
    a.V = V; a.L = L; a.B = B; a.D = D; a.ew = p->edge_weight_by_dst; a.ns = p->node_scale;
    a.in = p->X; a.ld_in = p->ldX; a.dz = p->dZ; a.ld_dz = p->lddZ; a.out = P;
    const Shape sh = pick_shape(D, rows_aligned(p->X, p->ldX) && rows_aligned(p->dZ, p->lddZ));
    launch_dcoeff_walk(sh, a, dim3((unsigned)(a.num_items + ceil_div(V, 256 / sh.lpr)), (unsigned)gy_dc), s);
    TFGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(basis_dcoeff_reduce1_kernel, dim3((unsigned)chunks, (unsigned)L), dim3(256), 0, s, g->views[0].rowptr, P, V, L, B, part2);
    TFGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(basis_dcoeff_reduce2_kernel, dim3((unsigned)ceil_div(L * B, 256)), dim3(256), 0, s, part2, (int)chunks, L * B, B,
                       p->dcoeff);
    TFGNN_LAUNCH_CHECK();
    g_basis_launches[2].fetch_add(3, std::memory_order_relaxed);
  }
  return TFGNN_OK;
}
