// Host description of one split-operand NT product, C = epilogue(A B^T) on SP16 operands (gemm_sp.hip gemm_sp_nt_kernel), and its
// one launch path.  The callers are the five entry points tfgnn_sp_gemm_nt, _sp, _dropout, _rows and _grouped (gemm_sp.hip) and
// the layer entry points tfgnn_mp_forward / tfgnn_mp_backward (mp_layer.hip): each fills the fields it has by name and leaves
// the rest at their defaults.  include/tfgnn.h documents every operand under the entry point that exposes it.
#pragma once
#include "common.hpp"

namespace tfgnn {

// The reduce pass of a split-K weight-gradient (TN) product, as sp_tn_reduce_body (gemm_sp.hip) takes it: filled by
// sp_tn_enqueue, run by sp_tn_reduce_kernel - or by the workgroups an NT launch carries behind its tiles (NtCall::tail).
struct TnReduceArgs {
  const float* partial;
  int splits;
  int64_t M, N;
  const float* ref;
  int64_t a_col0;
  int a_sb;
  float* C;
  int64_t group_rows, stride_group, stride_row, stride_col;
  int accumulate;
  int64_t slab;
  int ref_ld;  // 0: one reference scale per block (ref[blk]); > 0: one per (split, block) at ref[z * ref_ld + blk]
};

// A reduce pass whose launch its TN product left to the caller: the arguments and the workspace they point into (the product's
// partials, reference scales and trip words), which stays untouched until the pass has run.
struct TnReduceJob {
  unsigned blocks;  // workgroups an NT launch gives the pass (from the reduction's size); 0: nothing left to run
  TnReduceArgs args;
  const void* ws;
  size_t ws_bytes;
};

struct NtCall {
  int64_t M = 0, N = 0, K = 0;
  // operand A [M, K]
  const void* A = nullptr;
  int64_t lda_bytes = 0;
  const float* a_inv_scale = nullptr;
  int a_scale_block = 0;            // <= 0 or >= K: one block per row; < 0: one scale for the whole tensor
  const int32_t* a_rows = nullptr;  // row m of the product reads row a_rows[m] of A
  int64_t a_src_rows = 0;           // rows of A behind a_rows; <= 0: M
  // operand B [N, K] (grouped: one per group)
  const void* B = nullptr;
  int64_t ldb_bytes = 0;
  const float* b_inv_scale = nullptr;
  int64_t b_group_stride_bytes = -1;  // < 0: N ldb_bytes
  int64_t b_scale_group_stride = -1;  // < 0: N
  // result: fp32 C and / or the split form
  float* C = nullptr;
  int64_t ldc = 0;
  int accumulate = 0;
  void* out_sp = nullptr;
  int64_t ld_out_sp_bytes = 0;
  float* out_inv_scale = nullptr;
  // epilogue
  const float* bias = nullptr;
  int act = TFGNN_ACT_NONE;
  const float* mul = nullptr;
  int64_t ld_mul = 0;
  int act_of_saved = TFGNN_ACT_NONE;
  const float* saved = nullptr;
  int64_t ld_saved = 0;
  float saved_scale = 1.f;
  float dropout_rate = 0.f;
  uint64_t dropout_seed = 0;
  // row selection
  const uint8_t* tile_kmask = nullptr;
  const int32_t* row_map = nullptr;
  const int32_t* tile_table = nullptr;
  int64_t num_tiles_m = 0;
  int num_groups = 1;
  // optional: the reduce pass of a TN product enqueued BEFORE this call on the same stream, run by extra workgroups behind the
  // product's own (sp_nt_tail_blocks of them); a call that launches nothing (M = 0) gives the pass its own launch
  const TnReduceJob* tail = nullptr;
};

// checks the call, plans the in-launch K split and enqueues the product on s; TFGNN_OK or the code of the first check that fails
int sp_nt_enqueue(const NtCall& c, hipStream_t s);

// the reduce pass in a launch of its own (what a TN product without a carrier does)
int sp_tn_reduce_enqueue(const TnReduceJob& job, hipStream_t s);

// tfgnn_sp_gemm_tn with the reduce pass handed back: everything up to and including the product (and the armed repair pass) is
// enqueued on s, *job receives the pass.  Same checks, same workspace, same arithmetic as the stand-alone entry.
int sp_gemm_tn_product(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, int64_t a_first_col,
                        const float* d_a_inv_scale, int64_t a_total_cols, int a_scale_block, const void* d_B_sp, int64_t ldb_bytes,
                        int64_t b_first_col, const float* d_b_inv_scale, float* d_C, int64_t group_rows, int64_t stride_group,
                        int64_t stride_row, int64_t stride_col, int accumulate, void* d_workspace, size_t workspace_bytes,
                        TnReduceJob* job, hipStream_t s);

}  // namespace tfgnn
