// R-GCN block-diagonal decomposition (Schlichtkrull et al., eq. 4: W_l = blockdiag(Q_l^0 .. Q_l^{C-1})), the blocks applied
// inside the neighbour walk, once per run of one edge type.  Qb [L, di, H] holds the blocks banded (di = D / C, ho = H / C):
//   W_l[c*di + i, c*ho + j] = Qb[l, i, c*ho + j]
//   pre[v, h]    = m_v * sum_{e = (u -> v), type l} s_e * sum_i X[u, c(h)*di + i] * Qb[l, i, h]                 tfgnn_blockdiag_forward
//   dX[u, d]     = sum_{e = (u -> v), type l} s'_e * sum_j dPre[v, c(d)*ho + j] * Qb[l, d % di, c(d)*ho + j]    tfgnn_blockdiag_backward
//   dQb[l, i, h] = sum_{e = (u -> v) of type l} m_v * s_e * X[u, c(h)*di + i] * dPre[v, h]
// The contracts and the order of every sum are stated in include/tfgnn.h ("R-GCN block-diagonal decomposition"); DESIGN.md §5g
// has the byte model.
//
// The two walks follow the skeleton of node_walk.hpp (the range and the item epilogue written out here, see there) over a NODE view of the graph handle and that view's long-row plan (short
// rows: one lane group each; long rows: items of item_chunk_edges edges, one workgroup each; rows of several items: partial rows in
// the workspace and a second, small launch).  blockIdx.y walks windows of whole blocks: window w holds blocks [w*cw, (w+1)*cw), its
// lane group owns their input columns (the run sum) AND their output columns (the accumulator); the run sum changes hands
// through a slab of LDS that belongs to the lane group.  A lane group never spans two waves, so the hand-over needs no
// workgroup barrier.  dQb does not walk rows: the caller's edge lists are type-major already, so stage 1 takes chunks of 256
// consecutive list positions of one type and stage 2 adds the chunk partials of a type in chunk order.
#include "node_walk.hpp"

namespace tfgnn {
namespace {

constexpr int MAX_BLOCK = 64;  // widest block (D / C or H / C): a block lives inside one lane group's window
constexpr int DQ_CHUNK = 256;  // list positions per chunk of dQb's stage 1
constexpr int DQ_IT = 8;       // block rows i a lane accumulates at once in stage 1
constexpr int DQ_COLS = 64;    // output columns per stage-1 workgroup: one per lane of a wave

std::atomic<int64_t> g_blockdiag_launches[3];  // forward, dX, dQb

struct WalkArgs {  // the fields of NodeWalkArgs (node_walk.hpp) in this kernel's own order, then its own
  const int32_t* nodeptr;  // [V+1] the node view's row pointers
  const int32_t* coll;     // [E]   other end * L + type
  int64_t V;
  int L, C, H;
  int bi, bo;  // block width on the side the walk reads (forward di, dX ho) and on the side it writes (forward ho, dX di)
  int cw;      // blocks per window
  const float* qb;  // [L, di, H]
  const float* ew;  // [E] in the view's edge order, or NULL (= 1)
  const float* ns;  // [V] m_v (forward), or NULL (= 1)
  const float* in;  // forward X [V, D]; dX: dPre [V, H]
  int64_t ld_in;
  float* out;  // forward pre [V, H]; dX: dX [V, D]
  int64_t ld_out;
  float* partial;  // [num_partials, width_out]
  int width_out;
  int long_threshold, item_chunk_edges, num_items;
  const int32_t *item_row, *item_chunk, *item_slot;
};

// the lanes of a group run in one wave: what they wrote to the group's slab is visible to them after this
__device__ __forceinline__ void group_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// edges [beg, end) of one row -> acc += sum over the type runs (ascending) of (run sum) x (the type's blocks); the run sum is
// taken over the run's edges in order, run = fma(w_e, in, run); the blocks are applied with the block's inner index ascending.
// TR = false (forward): acc[h] = fma(run[c(h)*di + i], Qb[l, i, h], acc[h]);
// TR = true  (dX):      acc[d] = fma(run[c(d)*ho + j], Qb[l, d % di, c(d)*ho + j], acc[d]).
// lc: the lane's first local column (the same on both sides); c0: the window's first block.
template <int VEC, bool TR>
__device__ __forceinline__ void walk(const WalkArgs& a, int32_t beg, int32_t end, int c0, int lc, bool live_in, bool live_out,
                                     float* slab, float (&acc)[VEC]) {
  if (beg >= end) return;
  const int cb = lc / a.bo;  // the local block of the lane's output columns
  const float* in = a.in + c0 * a.bi + lc;
  float run[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) run[c] = 0.f;
  auto apply = [&](int l) {
    if (live_in) {
#pragma unroll
      for (int c = 0; c < VEC; ++c) slab[lc + c] = run[c];
    }
    group_sync();
    if (live_out) {
      const float* sl = slab + cb * a.bi;
      const float* q = a.qb + (int64_t)l * (TR ? a.bo : a.bi) * a.H;
      if constexpr (!TR) {
        q += c0 * a.bo + lc;
#pragma unroll 4
        for (int t = 0; t < a.bi; ++t) {
          const float r = sl[t];
          const Vec<VEC> w = load_vec<VEC>(q + (int64_t)t * a.H, true);
#pragma unroll
          for (int c = 0; c < VEC; ++c) acc[c] = fmaf(r, w.v[c], acc[c]);
        }
      } else {
        q += (int64_t)(lc - cb * a.bo) * a.H + (c0 + cb) * a.bi;  // row d % di, first column of block c(d)
#pragma unroll 4
        for (int t = 0; t < a.bi; ++t) {
          const float r = sl[t];
#pragma unroll
          for (int c = 0; c < VEC; ++c) acc[c] = fmaf(r, q[(int64_t)c * a.H + t], acc[c]);
        }
      }
    }
    group_sync();  // the next run writes the slab again
  };
  int cur = -1;
  int32_t cl = a.coll[beg];
  float w = a.ew ? a.ew[beg] : 1.f;
  Vec<VEC> x = load_vec<VEC>(in + (int64_t)(cl / a.L) * a.ld_in, live_in);
  for (int32_t e = beg; e < end; ++e) {
    const int32_t en = min(e + 1, end - 1);  // the next edge's row is in flight while this one is added
    const int32_t ncl = a.coll[en];
    const float nw = a.ew ? a.ew[en] : 1.f;
    const Vec<VEC> nx = load_vec<VEC>(in + (int64_t)(ncl / a.L) * a.ld_in, live_in);
    const int t = cl % a.L;
    if (t != cur) {
      if (cur >= 0) apply(cur);
      cur = t;
#pragma unroll
      for (int c = 0; c < VEC; ++c) run[c] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < VEC; ++c) run[c] = fmaf(w, x.v[c], run[c]);
    cl = ncl; w = nw; x = nx;
  }
  apply(cur);
}

// One launch, both kinds of work: workgroups [0, num_items) take one item of a long row each, the others 256 / LPR short rows.
template <int VEC, int LPR, bool TR>
__global__ void __launch_bounds__(256) blockdiag_rows_kernel(WalkArgs a) {
  constexpr int GROUPS = 256 / LPR;
  constexpr int PW = LPR * VEC;  // columns of a window, on either side
  __shared__ float slab[GROUPS][PW];
  __shared__ float red[GROUPS][PW];
  const int tid = threadIdx.x, group = tid / LPR, gl = tid % LPR;
  const int c0 = blockIdx.y * a.cw;
  const int nb = min(a.cw, a.C - c0);  // blocks of this window
  const int lc = gl * VEC;
  const bool live_in = lc < nb * a.bi, live_out = lc < nb * a.bo;
  float acc[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc[c] = 0.f;

  if ((int)blockIdx.x >= a.num_items) {  // short rows, in node order: one lane group per row
    const int64_t row = ((int64_t)blockIdx.x - a.num_items) * GROUPS + group;
    if (row >= a.V) return;
    const int32_t beg = a.nodeptr[row], end = a.nodeptr[row + 1];
    if (end - beg > a.long_threshold || !(live_in || live_out)) return;  // long rows: the item workgroups
    walk<VEC, TR>(a, beg, end, c0, lc, live_in, live_out, slab[group], acc);
    if (!live_out) return;
    const float m = a.ns ? a.ns[row] : 1.f;
    float* o = a.out + row * a.ld_out + c0 * a.bo + lc;
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0] * m, acc[1] * m, acc[2] * m, acc[3] * m);
    else *o = acc[0] * m;
    return;
  }

  const int item = blockIdx.x;
  const int64_t row = a.item_row[item];
  const int32_t rbeg = a.nodeptr[row], rend = a.nodeptr[row + 1];
  const int32_t ibeg = min(rend, rbeg + a.item_chunk[item] * a.item_chunk_edges);
  const int32_t iend = min(rend, ibeg + a.item_chunk_edges);
  const int per = (iend - ibeg + GROUPS - 1) / GROUPS;  // consecutive edges per lane group
  const int32_t beg = min(iend, ibeg + group * per), end = min(iend, beg + per);
  if (live_in || live_out) walk<VEC, TR>(a, beg, end, c0, lc, live_in, live_out, slab[group], acc);
#pragma unroll
  for (int c = 0; c < VEC; ++c) red[group][lc + c] = acc[c];
  __syncthreads();
  const int32_t slot = a.item_slot[item];
  const float m = (a.ns && slot < 0) ? a.ns[row] : 1.f;
  float* orow = slot < 0 ? a.out + row * a.ld_out : a.partial + (int64_t)slot * a.width_out;
  for (int f = tid; f < nb * a.bo; f += 256) {
    float s = red[0][f];
#pragma unroll
    for (int g = 1; g < GROUPS; ++g) s += red[g][f];
    orow[c0 * a.bo + f] = s * m;
  }
}

struct DqArgs {
  const int32_t* list_to_dst;  // [E] position in concat(adjacency_lists) -> position in the by-target order
  const int32_t* chunk_first;  // [num_chunks] first list position
  const int32_t* chunk_count;  // [num_chunks] 1 .. DQ_CHUNK list positions
  const int32_t* coll;         // [E] by target: source * L + type
  const int32_t* tgt;          // [E] by target: target
  int L, di, ho, H, itiles;
  const float* ew;  // [E] by target, or NULL
  const float* ns;  // [V] or NULL
  const float* X;
  int64_t ldX;
  const float* dpre;
  int64_t ld_dpre;
  float* part;  // [num_chunks, di, H]
};

// ---- dQb, stage 1: workgroup (chunk, tile of DQ_COLS columns x DQ_IT block rows).  Lane = column h; wave w takes the w-th
// quarter (ceil(n / 4) consecutive positions) of the chunk's n edges in list order: p[i] = fma(x[c(h)*di + i], g, p[i]) with
// g = (m_v * s_e) * dPre[v, h]; the four waves' sums are added in wave order. ----
__global__ void __launch_bounds__(256) blockdiag_dq_stage1_kernel(DqArgs a) {
  __shared__ float red[4][DQ_IT][DQ_COLS];
  const int chunk = blockIdx.x;
  const int ct = blockIdx.y / a.itiles, i0 = (blockIdx.y % a.itiles) * DQ_IT;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int h = ct * DQ_COLS + lane;
  const bool live = h < a.H;
  const int xc = live ? (h / a.ho) * a.di + i0 : 0;
  const int32_t first = a.chunk_first[chunk], n = a.chunk_count[chunk];
  const int per = (n + 3) / 4;
  const int kb = min(n, wave * per), ke = min(n, kb + per);
  float p[DQ_IT];
#pragma unroll
  for (int j = 0; j < DQ_IT; ++j) p[j] = 0.f;
  if (live) {
    for (int k = kb; k < ke; ++k) {
      const int32_t q = a.list_to_dst[first + k];
      const int64_t u = a.coll[q] / a.L, v = a.tgt[q];
      const float kf = (a.ns ? a.ns[v] : 1.f) * (a.ew ? a.ew[q] : 1.f);
      const float g = kf * a.dpre[v * a.ld_dpre + h];
      const float* xr = a.X + u * a.ldX + xc;
#pragma unroll
      for (int j = 0; j < DQ_IT; ++j)
        if (i0 + j < a.di) p[j] = fmaf(xr[j], g, p[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < DQ_IT; ++j) red[wave][j][lane] = p[j];
  __syncthreads();
  for (int f = threadIdx.x; f < DQ_IT * DQ_COLS; f += 256) {
    const int j = f / DQ_COLS, ln = f % DQ_COLS, hh = ct * DQ_COLS + ln;
    if (i0 + j >= a.di || hh >= a.H) continue;
    a.part[((int64_t)chunk * a.di + i0 + j) * a.H + hh] = ((red[0][j][ln] + red[1][j][ln]) + red[2][j][ln]) + red[3][j][ln];
  }
}

// stage 2: dQb[l, i, h] = the partials of the chunks of type l in chunk order (none: an exact 0)
__global__ void __launch_bounds__(256)
blockdiag_dq_stage2_kernel(const int32_t* __restrict__ type_chunk_ptr, const float* __restrict__ part, int n, float* __restrict__ dq) {
  const int l = blockIdx.y;
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  const int32_t c0 = type_chunk_ptr[l], c1 = type_chunk_ptr[l + 1];
  float s = 0.f;
  for (int32_t c = c0; c < c1; ++c) s += part[(int64_t)c * n + f];
  dq[(int64_t)l * n + f] = s;
}

struct Shape {
  bool vec;
  int lpr, cw;
};
// vector path: both block widths multiples of 4 and every row involved 16-byte aligned.  Of the lane groups of 16, 32 and 64
// lanes that can hold a block, the one whose windows need the fewest lanes in total (ties: the wider group).
inline Shape pick_shape(int C, int di, int ho, bool aligned) {
  Shape s{};
  s.vec = di % 4 == 0 && ho % 4 == 0 && aligned;
  const int unit = s.vec ? 4 : 1, bw = std::max(di, ho);
  int64_t best = -1;
  for (int lpr : {16, 32, 64}) {
    const int cw = std::min(C, lpr * unit / bw);
    if (cw < 1) continue;
    const int64_t lanes = ceil_div((int64_t)C, (int64_t)cw) * lpr;
    if (best < 0 || lanes <= best) {
      best = lanes;
      s.lpr = lpr;
      s.cw = cw;
    }
  }
  return s;
}

// the walk launch and, when some row has several items, the launch that adds their partial rows; `slot`: launch counter
template <bool TR>
int launch_rows(const Shape& sh, const WalkArgs& a, const GraphView& gv, int slot, hipStream_t s) {
  const dim3 grid((unsigned)(a.num_items + ceil_div(a.V, (int64_t)(256 / sh.lpr))), (unsigned)ceil_div(a.C, sh.cw));
  auto walk = [&] {
    dispatch_shape(sh.vec, sh.lpr, [&](auto vec, auto lpr) {
      hipLaunchKernelGGL((blockdiag_rows_kernel<decltype(vec)::value, decltype(lpr)::value, TR>), grid, dim3(256), 0, s, a);
    });
  };
  return launch_walk(walk, gv, a.partial, a.ns, a.width_out, a.out, a.ld_out, g_blockdiag_launches[slot], s);
}

// the limits on the three widths alone (no handle): TFGNN_OK or the error code, the message set
int check_widths(const char* who, int C, int D, int H) {
  TFGNN_REQUIRE(C >= 1, "%s: num_blocks = %d, the limit is num_blocks >= 1", who, C);
  TFGNN_REQUIRE(D >= 1 && H >= 1, "%s: D = %d, H = %d, the limit is D >= 1 and H >= 1", who, D, H);
  TFGNN_REQUIRE(D % C == 0 && H % C == 0, "%s: num_blocks = %d must divide D = %d and H = %d", who, C, D, H);
  if (D / C > MAX_BLOCK || H / C > MAX_BLOCK) {
    set_error("%s: blocks of %d x %d (D = %d, H = %d, num_blocks = %d) are above the limit D / num_blocks <= %d and H / num_blocks <= %d",
              who, D / C, H / C, D, H, C, MAX_BLOCK, MAX_BLOCK);
    return TFGNN_ERR_UNSUPPORTED;
  }
  if (C > 65535) {
    set_error("%s: num_blocks = %d is above the limit num_blocks <= 65535", who, C);
    return TFGNN_ERR_UNSUPPORTED;
  }
  return TFGNN_OK;
}

int check_limits(const char* who, const tfgnn_graph* g, int C, int D, int H) {
  const int rc = check_widths(who, C, D, H);
  if (rc) return rc;
  return check_graph(who, g);
}

}  // namespace
}  // namespace tfgnn

extern "C" size_t tfgnn_blockdiag_workspace_bytes(int C, int D, int H, int64_t partials_by_dst, int64_t partials_by_src,
                                                  int64_t num_chunks) {
  using namespace tfgnn;
  if (C < 1 || D < 1 || H < 1 || D % C || H % C || D / C > MAX_BLOCK || H / C > MAX_BLOCK || partials_by_dst < 0 ||
      partials_by_src < 0 || num_chunks < 0)
    return 0;
  const size_t fwd = align16((size_t)partials_by_dst * H * 4);
  const size_t bwd = align16((size_t)partials_by_src * D * 4) + align16((size_t)num_chunks * (D / C) * H * 4);
  return std::max(fwd, bwd);
}

extern "C" int tfgnn_blockdiag_launch_counts(int64_t* out_counts, int n) {
  using namespace tfgnn;
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_blockdiag_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i < 3 ? g_blockdiag_launches[i].load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

extern "C" int tfgnn_blockdiag_forward(const tfgnn_blockdiag_forward_args* p, void* stream) {
  using namespace tfgnn;
  const char* who = "tfgnn_blockdiag_forward";
  TFGNN_REQUIRE(p != nullptr && p->struct_size == sizeof(tfgnn_blockdiag_forward_args),
                "%s: args is NULL or was built against another header (struct_size)", who);
  const int rc = check_limits(who, p->graph, p->C, p->D, p->H);
  if (rc) return rc;
  const tfgnn_graph* g = p->graph;
  const int C = p->C, D = p->D, H = p->H, di = D / C, ho = H / C;
  if (g->V == 0) return TFGNN_OK;
  TFGNN_REQUIRE(p->Qb && p->X && p->pre, "%s: NULL pointer", who);
  TFGNN_REQUIRE(p->ldX >= D && p->ldpre >= H, "%s: a row stride is smaller than its row", who);
  const GraphView& gv = g->views[1];  // by target, all edge types of a node in one row
  const size_t need = (size_t)gv.plan.num_partials * H * 4;
  TFGNN_REQUIRE(need == 0 || (p->workspace && p->workspace_bytes >= need && (uintptr_t)p->workspace % 16 == 0),
                "%s: workspace too small or not 16-byte aligned: need %zu bytes", who, need);
  WalkArgs a{};
  fill_plan(a, gv);
  a.V = g->V; a.L = g->L; a.C = C; a.H = H; a.bi = di; a.bo = ho; a.qb = p->Qb; a.ew = p->edge_weight_by_dst; a.ns = p->node_scale;
  a.in = p->X; a.ld_in = p->ldX; a.out = p->pre; a.ld_out = p->ldpre; a.partial = (float*)p->workspace; a.width_out = H;
  const Shape sh = pick_shape(C, di, ho, rows_aligned(p->X, p->ldX) && rows_aligned(p->pre, p->ldpre) && (uintptr_t)p->Qb % 16 == 0);
  a.cw = sh.cw;
  return launch_rows<false>(sh, a, gv, 0, (hipStream_t)stream);
}

extern "C" int tfgnn_blockdiag_backward(const tfgnn_blockdiag_backward_args* p, void* stream) {
  using namespace tfgnn;
  const char* who = "tfgnn_blockdiag_backward";
  TFGNN_REQUIRE(p != nullptr && p->struct_size == sizeof(tfgnn_blockdiag_backward_args),
                "%s: args is NULL or was built against another header (struct_size)", who);
  const int rc = check_limits(who, p->graph, p->C, p->D, p->H);
  if (rc) return rc;
  const tfgnn_graph* g = p->graph;
  const int C = p->C, D = p->D, H = p->H, di = D / C, ho = H / C, L = g->L;
  const int64_t V = g->V, E = g->E;
  if (!p->dX && !p->dQb) return TFGNN_OK;
  hipStream_t s = (hipStream_t)stream;
  TFGNN_REQUIRE(V == 0 || (p->dPre && p->lddPre >= H), "%s: dPre is NULL or its row stride is smaller than H", who);
  TFGNN_REQUIRE(!p->dX || V == 0 || (p->Qb && p->lddX >= D), "%s: dX needs Qb and a row stride >= D", who);
  TFGNN_REQUIRE(!p->dQb || V == 0 || (p->X && p->ldX >= D), "%s: dQb needs X with a row stride >= D", who);
  const bool dq_work = p->dQb && V > 0 && E > 0;
  TFGNN_REQUIRE(!dq_work || (p->list_to_dst && p->chunk_first && p->chunk_count && p->type_chunk_ptr &&
                             p->num_chunks >= ceil_div(E, DQ_CHUNK) && p->num_chunks <= E),
                "%s: dQb needs the type-major tables (list_to_dst, chunk_first, chunk_count, type_chunk_ptr) with "
                "ceil(E / %d) <= num_chunks <= E", who, DQ_CHUNK);
  const GraphView& gs = g->views[3];  // by source
  const size_t o_part = align16((size_t)gs.plan.num_partials * D * 4);
  const size_t need = o_part + (dq_work ? align16((size_t)p->num_chunks * di * H * 4) : 0);
  TFGNN_REQUIRE(V == 0 || need == 0 || (p->workspace && p->workspace_bytes >= need && (uintptr_t)p->workspace % 16 == 0),
                "%s: workspace too small or not 16-byte aligned: need %zu bytes", who, need);
  char* ws = (char*)p->workspace;

  if (p->dX && V > 0) {
    WalkArgs a{};
    fill_plan(a, gs);
    a.V = V; a.L = L; a.C = C; a.H = H; a.bi = ho; a.bo = di; a.qb = p->Qb; a.ew = p->edge_weight_by_src;
    a.in = p->dPre; a.ld_in = p->lddPre; a.out = p->dX; a.ld_out = p->lddX; a.partial = (float*)ws; a.width_out = D;
    const Shape sh = pick_shape(C, di, ho, rows_aligned(p->dPre, p->lddPre) && rows_aligned(p->dX, p->lddX));
    a.cw = sh.cw;
    const int lrc = launch_rows<true>(sh, a, gs, 1, s);
    if (lrc) return lrc;
  }
  if (p->dQb) {
    const int64_t n = (int64_t)di * H;
    if (!dq_work) {  // no edge, no term: zeros
      TFGNN_HIP_CHECK(hipMemsetAsync(p->dQb, 0, (size_t)L * n * 4, s));
      return TFGNN_OK;
    }
    DqArgs a{};
    a.list_to_dst = p->list_to_dst; a.chunk_first = p->chunk_first; a.chunk_count = p->chunk_count;
    a.coll = g->coll_d; a.tgt = g->tgt_d;
    a.L = L; a.di = di; a.ho = ho; a.H = H; a.itiles = (int)ceil_div(di, DQ_IT);
    a.ew = p->edge_weight_by_dst; a.ns = p->node_scale; a.X = p->X; a.ldX = p->ldX; a.dpre = p->dPre; a.ld_dpre = p->lddPre;
    a.part = (float*)(ws + o_part);
    const int64_t gy = ceil_div(H, DQ_COLS) * a.itiles;
    TFGNN_REQUIRE(gy <= 65535, "%s: H = %d with blocks of %d rows needs more than 65535 tiles", who, H, di);
    hipLaunchKernelGGL(blockdiag_dq_stage1_kernel, dim3((unsigned)p->num_chunks, (unsigned)gy), dim3(256), 0, s, a);
    TFGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(blockdiag_dq_stage2_kernel, dim3((unsigned)ceil_div(n, (int64_t)256), (unsigned)L), dim3(256), 0, s, p->type_chunk_ptr,
                       a.part, (int)n, p->dQb);
    TFGNN_LAUNCH_CHECK();
    g_blockdiag_launches[2].fetch_add(2, std::memory_order_relaxed);
  }
  return TFGNN_OK;
}
