// Layer-level entry points (round 6; SURVEY.md section 8(b) planned them, VERDICT r5 "missing 1"): ONE call per message-passing
// layer and pass, for the formulation the benchmarked stacks run - the aggregate-first path of RGCN / GGNN / GNN_Edge_MLP
// without hidden layers and target states ("path A") on split operands:
//
//   forward   A[v, l, :] = s_{l,v} * sum_{(u,v) in A_l} x_u          csr_gather_reduce_kernel, written as the SP16 operand
//             out        = epilogue([A_0 | .. | A_{L-1}] @ [W_0; ..; W_{L-1}])   gemm_sp_nt_kernel (+ bias, activation, the next
//                                                                                 op's input dropout, the split form of the result)
//   backward  G[u, l, :] = sum_{(u,v) in A_l} w_e * d_pre[v, :]       the same gather over the by-source buckets
//             dW_l       = X^T G_l                                      gemm_sp_tn_kernel; its split reduction rides on the next launch
//             dX         = epilogue(G @ [W_0 | .. | W_{L-1}]^T)        gemm_sp_nt_kernel (+ gradient factors of the op below)
//             (over more than kCarryMaxRowTiles row tiles: dX first, then dW with its own reduction launch)
//
// i.e. the reference's message_passing.py:95-218 + gnn_edge_mlp.py:84-107 for one layer, and its share of
// tf.GradientTape.gradient (models/graph_task_model.py:347-357).  Host code only: each function walks the launch sequence the
// Python layer (tf2_gnn_amd/layers/message_passing/gnn_edge_mlp.py: _forward_A / _backward_A_f16x2) used to drive through
// four to six op-level calls - the same kernels with the same arguments, so results are bit-identical to the op-level route
// (tests/test_gpu_mp_entry.py) - without Python in between.  A binding from another framework needs
// these two calls per layer, the graph handle, and the loss.
#include <cstring>

#include "common.hpp"
#include "gemm_sp.hpp"
#include "tfgnn.h"

using namespace tfgnn;

// row tiles of the input-gradient product up to which tfgnn_mp_backward lets it carry the weight gradient's reduce pass:
// four rounds of one workgroup per CU
constexpr int64_t kCarryMaxRowTiles = 4 * 256;

extern "C" int tfgnn_mp_forward(const tfgnn_mp_forward_args* a, void* stream) {
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_mp_forward_args),
                "tfgnn_mp_forward: args is NULL or was built against another header (struct_size)");
  TFGNN_REQUIRE(a->kind == TFGNN_MP_AGGREGATE_FIRST, "tfgnn_mp_forward: unknown layer kind %d", a->kind);
  TFGNN_REQUIRE(a->graph && a->x && a->wt_sp && a->wt_inv_scale && a->agg_sp && a->agg_inv_scale && (a->out || a->out_sp),
                "tfgnn_mp_forward: NULL pointer");
  TFGNN_REQUIRE(a->view == TFGNN_VIEW_BY_DST_TYPED || a->view == TFGNN_VIEW_BY_DST_TYPED_PATTERN,
                "tfgnn_mp_forward: the forward pass gathers over the by-target typed buckets (view %d)", a->view);
  int64_t V = 0, E = 0;
  int L = 0;
  int rc = tfgnn_graph_dims(a->graph, &V, &L, &E);
  if (rc) return rc;
  const int64_t D = a->in_dim, H = a->hidden_dim, K = (int64_t)L * D;
  TFGNN_REQUIRE(V > 0 && L > 0 && D > 0 && H > 0, "tfgnn_mp_forward: empty layer");
  // 1. the aggregate, one SP16 row of L blocks per node (one scale per (node, type) bucket); buckets cut into several items
  //    are combined inside the gather's launch
  //    (agg_filled: the empty buckets' rows are in agg_sp / agg_inv_scale already and are left alone)
  rc = tfgnn_graph_gather_reduce_sp_keep_empty(a->graph, a->view, nullptr, nullptr, a->row_scale, a->x, a->ldx, (int)D, a->agg_sp, D * 4,
                                               a->agg_inv_scale, nullptr, a->workspace, a->workspace_bytes, a->agg_filled, stream);
  if (rc) return rc;
  // 2. W^T as the [H, L * D] operand, when the caller's copy is stale: a small-pass launch of its own.  A layer stack
  //    splits all its weights at the start of the pass instead (they do not change before the optimizer update) and hands
  //    in w = NULL: nothing is launched between the gather and the product
  if (a->w) {
    tfgnn_aux_job job;
    std::memset(&job, 0, sizeof(job));
    rc = tfgnn_sp_split_cols_job(a->w, H, K, H, a->wt_sp, a->ld_wt_sp_bytes, a->wt_inv_scale, &job);
    if (rc) return rc;
    rc = tfgnn_aux_launch(&job, 1, stream);
    if (rc) return rc;
  }
  // 3. the product with its epilogue
  NtCall c;
  c.M = V; c.N = H; c.K = K;
  c.A = a->agg_sp; c.lda_bytes = K * 4; c.a_inv_scale = a->agg_inv_scale; c.a_scale_block = (int)D;
  c.B = a->wt_sp; c.ldb_bytes = a->ld_wt_sp_bytes; c.b_inv_scale = a->wt_inv_scale;
  c.C = a->out; c.ldc = a->ld_out;
  c.out_sp = a->out_sp; c.ld_out_sp_bytes = a->ld_out_sp_bytes; c.out_inv_scale = a->out_inv_scale;
  c.bias = a->bias; c.act = a->act;
  c.dropout_rate = a->dropout_rate; c.dropout_seed = a->dropout_seed;
  c.tile_kmask = a->tile_kmask; c.row_map = a->row_map;
  return sp_nt_enqueue(c, (hipStream_t)stream);
}

extern "C" int tfgnn_mp_backward(const tfgnn_mp_backward_args* a, void* stream) {
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_mp_backward_args),
                "tfgnn_mp_backward: args is NULL or was built against another header (struct_size)");
  TFGNN_REQUIRE(a->kind == TFGNN_MP_AGGREGATE_FIRST, "tfgnn_mp_backward: unknown layer kind %d", a->kind);
  TFGNN_REQUIRE(a->graph && a->d_pre && a->wh_sp && a->wh_inv_scale && a->g_sp && a->g_inv_scale && (a->dx || a->dx_sp),
                "tfgnn_mp_backward: NULL pointer");
  TFGNN_REQUIRE(!a->dw || (a->x_sp && a->x_inv_scale), "tfgnn_mp_backward: the kernel gradients need the layer input as a split operand");
  int64_t V = 0, E = 0;
  int L = 0;
  int rc = tfgnn_graph_dims(a->graph, &V, &L, &E);
  if (rc) return rc;
  const int64_t D = a->in_dim, H = a->hidden_dim, K = (int64_t)L * H;
  TFGNN_REQUIRE(V > 0 && L > 0 && D > 0 && H > 0, "tfgnn_mp_backward: empty layer");
  // 1. G = [G_0 | .. | G_{L-1}]: d_pre summed over the out-edges of every (source, type) bucket
  //    (g_filled: as agg_filled of the forward call)
  rc = tfgnn_graph_gather_reduce_sp_keep_empty(a->graph, TFGNN_VIEW_BY_SRC_TYPED, nullptr, a->edge_weight, nullptr, a->d_pre, a->ld_d_pre,
                                               (int)H, a->g_sp, H * 4, a->g_inv_scale, nullptr, a->workspace, a->workspace_bytes,
                                               a->g_filled, stream);
  if (rc) return rc;
  // 2. the kernels as rows [W_0[d, :] | W_1[d, :] | ..] of the [D, L * H] operand, when the caller's copy is stale (see above)
  if (a->w) {
    tfgnn_aux_job job;
    std::memset(&job, 0, sizeof(job));
    rc = tfgnn_sp_split_rows_job(a->w, H, H, D * H, D, K, (int)K, a->wh_sp, a->ld_wh_sp_bytes, a->wh_inv_scale, nullptr, &job);
    if (rc) return rc;
    rc = tfgnn_aux_launch(&job, 1, stream);
    if (rc) return rc;
  }
  // 3. dW[l, d, h] = sum_v X[v, d] G[v, l, h]: element ((l, h), d) of G^T X scattered into the kernels' [L, D, H] layout.  The
  //    product only: its reduce pass rides on the launch of 4. (nothing on the critical path reads dW, and that launch leaves
  //    CUs free), so tn_workspace stays live through 4.  Only while the dX product is a few rounds of row tiles: past that
  //    nothing is hidden - the pass's workgroups start when the last tiles do - the launch it saves is below 3 % of the
  //    product, and the product that comes first behind the gather pays for it (2.3 M rows, 18 000 tiles: the TN product
  //    63 us slower, the NT product 39 us faster, the step 0.4 % up; NOTEBOOK 36): there the order stays dX, dW.
  const bool carry = a->dw && (V + 127) / 128 <= kCarryMaxRowTiles;
  TnReduceJob reduce{};
  if (carry) {
    const uintptr_t t0 = (uintptr_t)a->tn_workspace, t1 = t0 + a->tn_workspace_bytes;
    const uintptr_t w0 = (uintptr_t)a->workspace, w1 = w0 + a->workspace_bytes;
    TFGNN_REQUIRE(!(a->tn_workspace && a->workspace && t0 < w1 && w0 < t1), "tfgnn_mp_backward: tn_workspace overlaps workspace");
    rc = sp_gemm_tn_product(K, D, V, a->g_sp, K * 4, 0, a->g_inv_scale, K, (int)H, a->x_sp, a->ld_x_sp_bytes, 0, a->x_inv_scale, a->dw, H,
                            D * H, 1, H, 0, a->tn_workspace, a->tn_workspace_bytes, &reduce, (hipStream_t)stream);
    if (rc) return rc;
  }
  // 4. dX = G W^T with the gradient factors of the op below in the epilogue; rows in by-source pattern order when asked
  NtCall c;
  c.M = V; c.N = D; c.K = K;
  c.A = a->g_sp; c.lda_bytes = K * 4; c.a_inv_scale = a->g_inv_scale; c.a_scale_block = (int)H; c.a_rows = a->a_rows;
  c.B = a->wh_sp; c.ldb_bytes = a->ld_wh_sp_bytes; c.b_inv_scale = a->wh_inv_scale;
  c.C = a->dx; c.ldc = a->ld_dx; c.accumulate = a->accumulate;
  c.out_sp = a->dx_sp; c.ld_out_sp_bytes = a->ld_dx_sp_bytes; c.out_inv_scale = a->dx_inv_scale;
  c.mul = a->mul; c.ld_mul = a->ld_mul; c.act_of_saved = a->act_of_saved; c.saved = a->saved; c.ld_saved = a->ld_saved;
  c.saved_scale = a->saved_scale; c.dropout_rate = a->dropout_rate; c.dropout_seed = a->dropout_seed;
  c.tile_kmask = a->tile_kmask; c.row_map = a->row_map;
  c.tail = &reduce;  // (empty without dw, or when the product ran its own reduce pass)
  rc = sp_nt_enqueue(c, (hipStream_t)stream);
  // a product that was refused launched nothing: the reduce pass still has to run
  if (rc && reduce.blocks) (void)sp_tn_reduce_enqueue(reduce, (hipStream_t)stream);
  if (rc || !a->dw || carry) return rc;
  return tfgnn_sp_gemm_tn(K, D, V, a->g_sp, K * 4, 0, a->g_inv_scale, K, (int)H, a->x_sp, a->ld_x_sp_bytes, 0, a->x_inv_scale, a->dw, H, D * H, 1,
                          H, 0, a->tn_workspace, a->tn_workspace_bytes, stream);
}
