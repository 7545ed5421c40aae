// In-stream repair of a split-operand weight-gradient (TN) product whose spread guard tripped (tn_repair.hip).
// The one caller is sp_tn_enqueue (gemm_sp.hip), the launch path of tfgnn_sp_gemm_tn, tfgnn_sp_gemm_tn_wide and
// tfgnn_sp_gemm_tn_grouped: with repair armed it points the product kernels' guard flag at the tail of the call's own workspace
// (zeroed on the stream in front of them: tn_repair_begin) and enqueues sp_tn_repair_kernel between the product and the reduce pass.
//   plain products: ONE trip word per product.  The kernel returns at once while it is 0; otherwise it rewrites every split-K
//     slab in fp32 straight from the SP16 operands and sets the reference scales the reduce pass multiplies to 1.
//   grouped product: one trip word per K RANGE of the split table (the product stores with a stride of one word per range).  A
//     workgroup of range z looks at word z only and rewrites slab z only, with the references of range z; the other slabs of
//     the group stay as the product wrote them - the grouped reduce pass multiplies every slab by its own reference.
#pragma once
#include "common.hpp"

namespace tfgnn {

constexpr size_t kTnRepairTailBytes = 256;  // appended to the product's workspace while repair is armed: the trip word
// the grouped product's tail: one trip word per K range (at most kTnRepairGroupedMaxRanges per launch), then the word "this
// launch has been counted as repaired"; rounded up to 256 bytes
constexpr int kTnRepairGroupedMaxRanges = 512;
constexpr size_t kTnRepairGroupedTailBytes = ((size_t)(kTnRepairGroupedMaxRanges + 1) * sizeof(int) + 255) & ~(size_t)255;

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
  const int32_t* split_table;  // grouped product: [splits][2] = (first row, rows) of range z, instead of z k_chunk; else NULL
  int splits;
  float* ref;          // ref_per_split: [splits][a_nblk] (factors computed in the product kernel); else [a_nblk] (factor pass)
  int ref_per_split;
  int* trip;           // the product's trip word; grouped: [splits] words, one per range, and the counted word at
                       // trip[kTnRepairGroupedMaxRanges]
  unsigned long long* repaired;  // device counter "products repaired"
};

// is repair armed?  (initial state: environment TFGNN_GUARD_REPAIR, read once)
bool tn_repair_armed();
// zeroes the tail (tail_bytes from trip_word on) of a product about to be enqueued on s - one word: a memset node; the grouped
// product's whole tail: a small kernel (tn_repair.hip says why) - and counts the product as armed
int tn_repair_begin(int* trip_word, size_t tail_bytes, hipStream_t s);
// sp_tn_repair_kernel on s (a.repaired is filled in here)
int tn_repair_enqueue(TnRepairArgs a, hipStream_t s);

}  // namespace tfgnn
