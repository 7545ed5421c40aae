// In-stream repair of a split-operand weight-gradient (TN) product whose spread guard tripped (tn_repair.hip).
// sp_gemm_tn_impl (gemm_sp.hip) is the only caller: with repair armed it points the product kernels' guard flag at a word in the
// tail of its own workspace (zeroed by a memset node in front of them) and enqueues sp_tn_repair_kernel between the product and
// the reduce pass.  The kernel returns at once while the word is 0; otherwise it rewrites every split-K slab in fp32 straight
// from the SP16 operands and sets the reference scales the reduce pass multiplies to 1.
#pragma once
#include "common.hpp"

namespace tfgnn {

constexpr size_t kTnRepairTailBytes = 256;  // appended to the product's workspace while repair is armed: the trip word

struct TnRepairArgs {
  int64_t M, N, K;     // the product's own M (not padded to the tile), N % 64 == 0
  const uint8_t* A;    // SP16, rows = k; already advanced to the product's first column (a multiple of 16)
  int64_t lda;
  const uint8_t* B;
  int64_t ldb;
  const float* inv_a;  // [K][a_nblk]
  const float* inv_b;  // [K] or NULL (scales 1)
  int a_sb;
  int64_t a_col0;
  int a_nblk;
  float* partial;      // [splits][slab]
  int64_t slab;
  int64_t k_chunk;     // rows of K per split: split z covers [z k_chunk, min(K, (z + 1) k_chunk))
  int splits;
  float* ref;          // ref_per_split: [splits][a_nblk] (factors computed in the product kernel); else [a_nblk] (factor pass)
  int ref_per_split;
  const int* trip;     // the product's trip word
  unsigned long long* repaired;  // device counter "products repaired"
};

// is repair armed?  (initial state: environment TFGNN_GUARD_REPAIR, read once)
bool tn_repair_armed();
// memset node that zeroes the trip word of a product about to be enqueued on s; counts the product as armed
int tn_repair_begin(int* trip_word, hipStream_t s);
// sp_tn_repair_kernel on s (a.repaired is filled in here)
int tn_repair_enqueue(TnRepairArgs a, hipStream_t s);

}  // namespace tfgnn
