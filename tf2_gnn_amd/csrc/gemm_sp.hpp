// Host description of one split-operand NT product, C = epilogue(A B^T) on SP16 operands (gemm_sp.hip gemm_sp_nt_kernel), and its
// one launch path.  The callers are the five entry points tfgnn_sp_gemm_nt, _sp, _dropout, _rows and _grouped (gemm_sp.hip) and
// the layer entry points tfgnn_mp_forward / tfgnn_mp_backward (mp_layer.hip): each fills the fields it has by name and leaves
// the rest at their defaults.  include/tfgnn.h documents every operand under the entry point that exposes it.
#pragma once
#include "common.hpp"

namespace tfgnn {

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
};

// checks the call, plans the in-launch K split and enqueues the product on s; TFGNN_OK or the code of the first check that fails
int sp_nt_enqueue(const NtCall& c, hipStream_t s);

}  // namespace tfgnn
