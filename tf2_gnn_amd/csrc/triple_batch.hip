// One mini-batch of link-prediction triples, built on the device (include/tfgnn.h "Triple batches"): a chunk of a fold's
// positives plus fresh negatives -> the triples in global ids, the distinct endpoints in increasing id (the seed list the
// neighbour sampler takes) and the triples in the batch's local ids (ranks in that list = rows of the sampled batch).
//
// tfgnn_triple_batch_build enqueues 6 launches, every grid sized from B, K, V and the seed capacity - S, the number of
// distinct endpoints, exists on the device only:
//   build      one thread per output row: a positive is gathered from the store, a negative is drawn from its positive
//              (read from the store, not from the output) with the words of tfgnn_triples_draw_negatives; the row is
//              written and table[endpoint] = kMarked where it was -1 (plain stores of one value: idempotent)
//   count      scan over the table: marked entries per chunk of 1024 ids
//   scan       ONE workgroup: scan of those counts (carry across rounds of 256 chunks), S, the overflow bit
//   assign     scan over the table again: a marked id takes its rank among the marked - increasing global id - and goes
//              to `seeds`; ids beyond the capacity go back to -1
//   translate  local_triples: endpoints through the table; the bad-id and bad-endpoint bits
//   restore    table[seeds[i]] = -1
// Integers only.  The only atomic is atomicOr on the status word.  Every read of the store and of the table goes through
// an index checked against its size; every write is below a capacity.
#include <atomic>

#include "common.hpp"
#include "scan.hpp"

namespace tfgnn {
namespace {

constexpr int kThreads = kScanThreads;
constexpr int kMaxBlocks = 2048;
constexpr int32_t kMarked = -2;

std::atomic<int64_t> g_triple_batch_launches;

// workspace, in int32 words: the table [V rounded up to 4], the id chunk offsets [ceil(V / 1024) + 1]
struct Layout {
  int64_t table, vchunk_off, words;
};
inline Layout layout(int64_t V) {
  Layout w;
  auto up4 = [](int64_t n) { return (n + 3) / 4 * 4; };
  w.table = 0;
  w.vchunk_off = up4(V);
  w.words = w.vchunk_off + up4(ceil_div(V, kScanChunk) + 1);
  return w;
}

struct Params {
  int32_t V, P, B, K, N, cap;
  DropoutKey key;
  const int32_t* positives;
  const int32_t* positive_ids;
  int32_t* triples;
  int32_t* local;
  int32_t* seeds;
  int32_t* meta;  // status, S
  int32_t* table;
  int32_t* vchunk_off;
};

// the store row of output row e (a positive: itself; negative j = e - B: positive j / K of the batch); false: a
// positive_ids entry outside [0, P)
__device__ __forceinline__ bool store_row(const Params& Q, int32_t e, int32_t* u, int32_t* t, int32_t* v) {
  const int32_t i = e < Q.B ? e : (int32_t)((uint32_t)(e - Q.B) / (uint32_t)Q.K);
  const int32_t pid = Q.positive_ids[i];
  if ((uint32_t)pid >= (uint32_t)Q.P) return false;
  const int32_t* __restrict__ row = Q.positives + 3 * (int64_t)pid;
  *u = row[0];
  *t = row[1];
  *v = row[2];
  return true;
}

__global__ void __launch_bounds__(kThreads) triple_batch_build_kernel(const Params Q) {
  const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (tid == 0) {
    Q.meta[0] = 0;
    Q.meta[1] = 0;
  }
  for (int64_t e = tid; e < Q.N; e += (int64_t)gridDim.x * kThreads) {
    int32_t u = -1, t = -1, v = -1;
    const bool ok = store_row(Q, (int32_t)e, &u, &t, &v);
    if (ok && e >= Q.B) {  // the draw of tfgnn_triples_draw_negatives (use_epoch = 0) for negative j
      const uint64_t j = (uint64_t)(e - Q.B);
      const uint32_t a = dropout_word(Q.key, 2 * j);
      const uint32_t b = dropout_word(Q.key, 2 * j + 1);
      const bool target = (a >> 31) != 0;
      const uint32_t old = (uint32_t)(target ? v : u);
      const uint32_t draw = (uint32_t)(((uint64_t)b * (uint32_t)(Q.V - 1)) >> 32);  // in [0, V - 1)
      const int32_t node = (int32_t)(draw + (draw >= old ? 1u : 0u));
      if (target) v = node; else u = node;
    }
    int32_t* __restrict__ row = Q.triples + 3 * e;
    row[0] = u;
    row[1] = t;
    row[2] = v;
    if (!ok) continue;
    if ((uint32_t)u < (uint32_t)Q.V && Q.table[u] == -1) Q.table[u] = kMarked;
    if ((uint32_t)v < (uint32_t)Q.V && Q.table[v] == -1) Q.table[v] = kMarked;
  }
}

__global__ void __launch_bounds__(kThreads) triple_batch_count_kernel(const Params Q) {
  __shared__ int32_t wave_sums[kThreads / 64];
  count_marked_chunks(Q.table, Q.V, kMarked, Q.vchunk_off, wave_sums);
}

__global__ void __launch_bounds__(kThreads) triple_batch_scan_kernel(const Params Q) {
  __shared__ int32_t wave_sums[kThreads / 64];
  const int64_t chunks = ((int64_t)Q.V + kScanChunk - 1) / kScanChunk;
  const int32_t total = scan_chunk_totals(Q.vchunk_off, chunks, wave_sums);
  if (threadIdx.x == 0) {
    if (total > Q.cap) atomicOr(Q.meta, TFGNN_TRIPLE_BATCH_SEED_OVERFLOW);
    Q.meta[1] = min(total, Q.cap);
  }
}

__global__ void __launch_bounds__(kThreads) triple_batch_assign_kernel(const Params Q) {
  __shared__ int32_t wave_sums[kThreads / 64];
  assign_marked_chunks(Q.table, Q.V, kMarked, Q.vchunk_off, 0, Q.cap, Q.seeds, wave_sums);
}

__global__ void __launch_bounds__(kThreads) triple_batch_translate_kernel(const Params Q) {
  int status = 0;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < Q.N; e += (int64_t)gridDim.x * kThreads) {
    int32_t u, t, v;
    int32_t* __restrict__ out = Q.local + 3 * e;
    if (!store_row(Q, (int32_t)e, &u, &t, &v)) {
      status |= TFGNN_TRIPLE_BATCH_BAD_POSITIVE_ID;
      out[0] = out[1] = out[2] = -1;
      continue;
    }
    const int32_t* __restrict__ row = Q.triples + 3 * e;  // the endpoints as written (a negative's drawn node included)
    u = row[0];
    v = row[2];
    const bool u_ok = (uint32_t)u < (uint32_t)Q.V, v_ok = (uint32_t)v < (uint32_t)Q.V;
    if (!(u_ok && v_ok)) status |= TFGNN_TRIPLE_BATCH_BAD_ENDPOINT;
    out[0] = u_ok ? Q.table[u] : -1;  // -1 as well for an endpoint beyond the seed capacity
    out[1] = t;
    out[2] = v_ok ? Q.table[v] : -1;
  }
  if (status) atomicOr(Q.meta, status);
}

__global__ void __launch_bounds__(kThreads) triple_batch_restore_kernel(const Params Q) {
  const int32_t n = min(Q.meta[1], Q.cap);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int32_t v = Q.seeds[i];
    if ((uint32_t)v < (uint32_t)Q.V) Q.table[v] = -1;
  }
}

}  // namespace
}  // namespace tfgnn

using namespace tfgnn;

extern "C" int tfgnn_triple_batch_launch_counts(int64_t* out_counts, int n) {
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_triple_batch_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i == 0 ? g_triple_batch_launches.load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}

extern "C" size_t tfgnn_triple_batch_workspace_bytes(int64_t num_nodes) {
  if (num_nodes < 1 || num_nodes >= ((int64_t)1 << 31)) return 0;
  return (size_t)layout(num_nodes).words * sizeof(int32_t);
}

extern "C" int tfgnn_triple_batch_build(const tfgnn_triple_batch_args* a, void* stream_) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TFGNN_REQUIRE(a != nullptr && a->struct_size == sizeof(tfgnn_triple_batch_args),
                "tfgnn_triple_batch_build: args is NULL or was built against another header (struct_size)");
  const int64_t B = a->batch_size, K = a->negatives_per_positive, V = a->num_nodes;
  TFGNN_REQUIRE(B >= 1, "tfgnn_triple_batch_build: empty batch (no positive)");
  TFGNN_REQUIRE(K >= 0, "tfgnn_triple_batch_build: negatives_per_positive must be >= 0");
  TFGNN_REQUIRE(B <= ((int64_t)1 << 30) && K <= ((int64_t)1 << 30) && B * (1 + K) <= ((int64_t)1 << 30),
                "tfgnn_triple_batch_build: more than 2^30 triples in the batch");
  TFGNN_REQUIRE(a->num_positives >= 1 && a->num_positives < kLimit,
                "tfgnn_triple_batch_build: the store must hold P positives, P in [1, 2^31)");
  TFGNN_REQUIRE(V >= 1 && V < kLimit, "tfgnn_triple_batch_build: V must be in [1, 2^31)");
  TFGNN_REQUIRE(K == 0 || V >= 2, "tfgnn_triple_batch_build: a negative needs a second node (V >= 2)");
  TFGNN_REQUIRE(a->seed_capacity >= 1, "tfgnn_triple_batch_build: the seed capacity must be at least 1");
  TFGNN_REQUIRE(a->positives && a->positive_ids && a->triples && a->local_triples && a->seeds && a->meta && a->workspace,
                "tfgnn_triple_batch_build: NULL pointer");
  const Layout lay = layout(V);
  TFGNN_REQUIRE((uintptr_t)a->workspace % 16 == 0 && a->workspace_bytes >= (size_t)lay.words * sizeof(int32_t),
                "tfgnn_triple_batch_build: the workspace is too small or not 16-byte aligned (tfgnn_triple_batch_workspace_bytes)");

  Params Q;
  memset(&Q, 0, sizeof(Q));
  const int64_t N = B * (1 + K);
  Q.V = (int32_t)V;
  Q.P = (int32_t)a->num_positives;
  Q.B = (int32_t)B;
  Q.K = (int32_t)K;
  Q.N = (int32_t)N;
  Q.cap = (int32_t)std::min<int64_t>(a->seed_capacity, V);  // no more than V distinct endpoints exist
  Q.key = dropout_key(a->seed, 0.f);  // the key words alone; use_epoch = 0: the epoch word is not read
  Q.key.epoch = nullptr;
  Q.positives = a->positives;
  Q.positive_ids = a->positive_ids;
  Q.triples = a->triples;
  Q.local = a->local_triples;
  Q.seeds = a->seeds;
  Q.meta = a->meta;
  int32_t* ws = static_cast<int32_t*>(a->workspace);
  Q.table = ws + lay.table;
  Q.vchunk_off = ws + lay.vchunk_off;

  hipStream_t stream = (hipStream_t)stream_;
  const dim3 block(kThreads);
  const unsigned row_grid = scan_strided_grid(N, kThreads, kMaxBlocks);
  const unsigned id_grid = scan_strided_grid(V, kScanChunk, kMaxBlocks);
  hipLaunchKernelGGL(triple_batch_build_kernel, dim3(row_grid), block, 0, stream, Q);
  hipLaunchKernelGGL(triple_batch_count_kernel, dim3(id_grid), block, 0, stream, Q);
  hipLaunchKernelGGL(triple_batch_scan_kernel, dim3(1), block, 0, stream, Q);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(triple_batch_assign_kernel, dim3(id_grid), block, 0, stream, Q);
  hipLaunchKernelGGL(triple_batch_translate_kernel, dim3(row_grid), block, 0, stream, Q);
  hipLaunchKernelGGL(triple_batch_restore_kernel, dim3(scan_strided_grid(Q.cap, kThreads, kMaxBlocks)), block, 0, stream, Q);
  TFGNN_LAUNCH_CHECK();
  g_triple_batch_launches.fetch_add(6, std::memory_order_relaxed);
  return TFGNN_OK;
}
