// R-GCN basis decomposition (Schlichtkrull et al., eq. 3: W_l = sum_b a[l,b] V_b), aggregate first:
//   Z[v, b, :] = m_v * sum_{e = (u -> v), type l} s_e * a[l,b] * X[u, :]          tfgnn_basis_gather_forward
//   out        = act(Z.reshape(V, B*D) @ [V_0; ...; V_{B-1}])                      (the existing products)
// and the two reverse passes of the gather (tfgnn_basis_gather_backward).  The contracts and the order of every sum are
// stated in include/tfgnn.h ("R-GCN basis decomposition"); DESIGN.md has the byte model.
//
// All three walks run on the skeleton of node_walk.hpp over a NODE view of the graph handle and that view's long-row plan (short
// rows: one lane group each, LPR lanes over the feature columns, VEC floats each; long rows: items of item_chunk_edges edges,
// one workgroup each; rows of several items: partial rows in the workspace and a second, small launch).  The coefficient walk
// uses the ranges alone: it writes per run, not per row.
// blockIdx.y walks the feature windows (LPR * VEC columns) and, in the forward and coefficient walks, the tiles of bases.
#include "node_walk.hpp"

namespace tfgnn {
namespace {

constexpr int FWD_BT = 8;      // bases a lane accumulates at once in the forward walk (FWD_BT * VEC registers)
constexpr int DC_BT = 16;      // bases per tile of the coefficient walk (one dot product each)
constexpr int RED_NODES = 1024;  // nodes per workgroup of the coefficient reduction's first stage
constexpr int MAX_D = 1 << 20;

std::atomic<int64_t> g_basis_launches[3];  // forward, dX, dcoeff

struct BasisArgs : NodeWalkArgs {
  int B, D;
  const float* coeff;  // [L, B]
  const float* in;     // forward, dcoeff: X [V, D]; dX: dZ [V, B*D]
  int64_t ld_in;
  const float* dz;  // dcoeff: dZ
  int64_t ld_dz;
  float* out;  // forward: Z; dX: dX; dcoeff: P [E, B] (dot products at the first edge of every run)
  int64_t ld_out;
};

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

  const GroupRange r = group_range<GROUPS>(a, blockIdx.x, group);
  const float* ns = FWD ? a.ns : nullptr;
  if (r.whole_row) {  // a short row: one lane group, no LDS
    if (r.row < 0 || !live) return;
    if constexpr (FWD) forward_walk<VEC>(a, r.beg, r.end, d, live, b0, acc);
    else dx_walk<VEC>(a, r.beg, r.end, d, live, acc[0]);
    const float m = ns ? ns[r.row] : 1.f;
    float* orow = a.out + r.row * a.ld_out;
#pragma unroll
    for (int j = 0; j < NACC; ++j)
      if (!FWD || b0 + j < a.B) store_vec<VEC>(orow + (int64_t)(b0 + j) * a.D + d, acc[j], m);
    return;
  }
  if (live) {
    if constexpr (FWD) forward_walk<VEC>(a, r.beg, r.end, d, live, b0, acc);
    else dx_walk<VEC>(a, r.beg, r.end, d, live, acc[0]);
  }
  item_epilogue<VEC, LPR, NACC>(a, r, red, acc, ns, a.out, a.ld_out, width, NACC * PW, [&](int f) {
    const int j = f / PW, dd = win * PW + f % PW;
    return Column<int64_t>{dd < a.D && (!FWD || b0 + j < a.B), (int64_t)(b0 + j) * a.D + dd};
  });
}

// ---- dcoeff, walk: for every run of one edge type inside the edges a lane group walks, P[first edge of the run, b] =
// m_v * <run sum of s_e X[u_e, :], dZ[v, b, :]>.  The run sum is never stored.  blockIdx.y: tile of DC_BT bases. ----
template <int VEC, int LPR>
__global__ void __launch_bounds__(256) basis_dcoeff_walk_kernel(BasisArgs a) {
  constexpr int GROUPS = 256 / LPR;
  constexpr int PW = LPR * VEC;
  const int tid = threadIdx.x, group = tid / LPR, gl = tid % LPR;
  const int b0 = blockIdx.y * DC_BT;
  const GroupRange r = group_range<GROUPS>(a, blockIdx.x, group);
  if (r.row < 0) return;
  const int32_t end = r.end;
  const float m = a.ns ? a.ns[r.row] : 1.f;
  const float* zrow = a.dz + r.row * a.ld_dz;
  // every lane of the group runs the same loops (the shuffles below stay inside the group)
  int32_t e = r.beg;
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

// the rows walk and, when some row has several items, the launch that adds their partial rows; `slot`: launch counter
template <bool FWD>
int launch_rows(const Shape& sh, const BasisArgs& a, const GraphView& gv, int64_t gy, int slot, hipStream_t s) {
  const dim3 grid((unsigned)(a.num_items + ceil_div(a.V, 256 / sh.lpr)), (unsigned)gy);
  auto walk = [&] {
    dispatch_shape(sh.vec, sh.lpr, [&](auto vec, auto lpr) {
      hipLaunchKernelGGL((basis_rows_kernel<decltype(vec)::value, decltype(lpr)::value, FWD>), grid, dim3(256), 0, s, a);
    });
  };
  return launch_walk(walk, gv, a.partial, FWD ? a.ns : nullptr, FWD ? a.B * a.D : a.D, a.out, a.ld_out, g_basis_launches[slot], s);
}
void launch_dcoeff_walk(const Shape& sh, const BasisArgs& a, dim3 grid, hipStream_t s) {
  dispatch_shape(sh.vec, sh.lpr, [&](auto vec, auto lpr) {
    hipLaunchKernelGGL((basis_dcoeff_walk_kernel<decltype(vec)::value, decltype(lpr)::value>), grid, dim3(256), 0, s, a);
  });
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
  return check_graph(who, g);
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
  return launch_rows<true>(sh, a, gv, gy, 0, (hipStream_t)stream);
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
    const int rc_dx = launch_rows<false>(sh, a, gs, ceil_div(D, pw), 1, s);
    if (rc_dx) return rc_dx;
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
