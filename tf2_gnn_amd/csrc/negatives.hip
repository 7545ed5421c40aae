// Link prediction, the per-epoch part that used to run on the host: drawing the negatives of a fold's triples and rebuilding
// the triple tables tfgnn_distmult_backward walks (include/tfgnn.h "Negative sampling and triple tables on the device" has the
// contract).  Integers only - no float arithmetic in this file.
//
// tfgnn_triples_draw_negatives: one launch, one thread per negative.  Negative j hashes the generator's words 2 j and 2 j + 1
// of (seed, epoch) - the dropout mask generator of common.hpp, epoch word read once per kernel - into a coin and a node, and
// writes its whole row.
//
// tfgnn_triple_tables_build: a stable sort of the 2 N (node, entry) keys, and of the N keys by relation, plus row pointers -
// the scheme of graph.hip's bucketing (its own copy: graph.hip sorts two sides of composite keys per launch and its compiled
// code is pinned by tests): LSD radix sort, 9-bit digits, 8192 keys per workgroup, per-tile digit histograms in a
// [digit][tile] table; a scatter workgroup takes the column prefix of its tile and the digit bases from that table itself,
// a wave owns 1024 consecutive keys of the tile and ranks them with ballots.  No global atomic anywhere; the only atomics are
// the LDS histogram counts, whose sums do not depend on their order.  The first pass reads its keys out of the triples
// (entry i = 2 e + role holds the node of that role of triple e), the last one writes the payloads - the entries - straight
// into the output table; the row pointers are a binary search per row over the sorted keys.  A hub node is just many equal
// keys: no kernel walks a node's entries.
#include <atomic>

#include "common.hpp"

namespace tfgnn {
namespace {

std::atomic<int64_t> g_negatives_launches[2];  // draws, table builds

// ---- the draw ------------------------------------------------------------------------------------------------------------
constexpr int DRAW_THREADS = 256;

__global__ void __launch_bounds__(DRAW_THREADS)
draw_negatives_kernel(int32_t* __restrict__ triples, int64_t P, uint32_t K, int64_t negatives, uint32_t other_nodes,
                      const DropoutKey key) {
  const DropoutKey k = dropout_resolve(key);
  for (int64_t j = (int64_t)blockIdx.x * DRAW_THREADS + threadIdx.x; j < negatives; j += (int64_t)gridDim.x * DRAW_THREADS) {
    const int64_t p = (int64_t)((uint32_t)j / K);  // j < 2^30
    const int32_t u = triples[3 * p], t = triples[3 * p + 1], v = triples[3 * p + 2];
    const uint32_t a = dropout_word(k, (uint64_t)(2 * j));
    const uint32_t b = dropout_word(k, (uint64_t)(2 * j + 1));
    const bool target = (a >> 31) != 0;
    const uint32_t old = (uint32_t)(target ? v : u);
    const uint32_t draw = (uint32_t)(((uint64_t)b * other_nodes) >> 32);  // in [0, V - 1)
    const int32_t node = (int32_t)(draw + (draw >= old ? 1u : 0u));
    int32_t* __restrict__ row = triples + 3 * (P + j);
    row[0] = target ? u : node;
    row[1] = t;
    row[2] = target ? node : v;
  }
}

// ---- the tables: stable LSD radix sort of 32-bit keys with a 32-bit payload ---------------------------------------------------
constexpr int TS_THREADS = 512;
constexpr int TS_ROUNDS = 16;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_WAVE_KEYS = 64 * TS_ROUNDS;     // consecutive keys per wave
constexpr int TS_TILE = TS_THREADS * TS_ROUNDS;  // 8192 keys per workgroup
constexpr int TS_DIGIT_BITS = 9;
constexpr int TS_RADIX = 1 << TS_DIGIT_BITS;     // 512 = one digit per thread
static_assert(TS_RADIX == TS_THREADS, "one digit per thread");

// key of position idx before the first pass.  by_node: idx = 2 e + role, the node of that role; else idx = e, the relation
__device__ __forceinline__ uint32_t triple_key(const int32_t* __restrict__ triples, int64_t idx, int by_node) {
  return (uint32_t)(by_node ? triples[3 * (idx >> 1) + 2 * (idx & 1)] : triples[3 * idx + 1]);
}

// hist[digit * nblk_ld + tile] = number of keys of the tile with that digit.  kin == NULL: the keys come out of the triples
__global__ void __launch_bounds__(TS_THREADS)
ts_hist_kernel(const uint32_t* __restrict__ kin, const int32_t* __restrict__ triples, int by_node, int64_t n, int shift,
               int32_t* __restrict__ hist, int nblk_ld) {
  __shared__ int32_t h[TS_RADIX];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * TS_TILE;
#pragma unroll 4
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const int64_t idx = base + r * TS_THREADS + tid;
    if (idx < n) {
      const uint32_t key = kin ? kin[idx] : triple_key(triples, idx, by_node);
      atomicAdd(&h[(int)((key >> shift) & (TS_RADIX - 1))], 1);  // LDS; a count: any order
    }
  }
  __syncthreads();
  hist[(int64_t)tid * nblk_ld + blockIdx.x] = h[tid];
}

// stable scatter of one digit: keys keep their input order inside a digit (tile, then wave, round, lane = index order).
// kin == NULL (first pass): keys out of the triples, payload = the key's index.  kout == NULL: the sorted keys are not kept.
__global__ void __launch_bounds__(TS_THREADS)
ts_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ pin, const int32_t* __restrict__ triples,
                  int by_node, int64_t n, int shift, const int32_t* __restrict__ hist, int nblk, int nblk_ld,
                  uint32_t* __restrict__ kout, uint32_t* __restrict__ pout) {
  __shared__ uint32_t wbase[TS_WAVES][TS_RADIX];  // per wave: digit counts, then running output positions
  __shared__ uint32_t wtot[TS_WAVES];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  volatile uint32_t* mine_base = &wbase[wave][0];
#pragma unroll
  for (int i = 0; i < TS_RADIX / 64; ++i) mine_base[lane + 64 * i] = 0;
  __builtin_amdgcn_wave_barrier();
  // 1. keys into registers; digit counts of this wave (one leader lane per digit and round adds the group size)
  const int64_t wave0 = (int64_t)blockIdx.x * TS_TILE + (int64_t)wave * TS_WAVE_KEYS;
  const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  uint32_t key[TS_ROUNDS], pl[TS_ROUNDS];
  int32_t info[TS_ROUNDS];  // rank | group size << 8 | valid << 16
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const int64_t idx = wave0 + r * 64 + lane;
    const bool valid = idx < n;
    key[r] = valid ? (kin ? kin[idx] : triple_key(triples, idx, by_node)) : 0u;
    pl[r] = valid ? (kin ? pin[idx] : (uint32_t)idx) : 0u;
  }
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const bool valid = wave0 + r * 64 + lane < n;
    const int d = (int)((key[r] >> shift) & (TS_RADIX - 1));
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < TS_DIGIT_BITS; ++b) {
      const unsigned long long m = __ballot((d >> b) & 1);
      peers &= ((d >> b) & 1) ? m : ~m;
    }
    const int rank = __popcll(peers & lt_mask);
    const int cnt = __popcll(peers);
    info[r] = valid ? (rank | (cnt << 8) | (1 << 16)) : 0;
    if (valid && rank == 0) mine_base[d] = mine_base[d] + cnt;  // leaders of one round hold distinct digits
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // 2. thread d: keys with digit d in the tiles before this one + the digit's global base -> the waves' first positions
  //    (unsigned: the total is 2^31 at N = 2^30; a position never exceeds 2^31 - 1)
  uint32_t tot = 0, before = 0;
  {
    const int32_t* __restrict__ row = hist + (int64_t)tid * nblk_ld;
    const int me = (int)blockIdx.x;
    for (int b0 = 0; b0 < nblk; b0 += 16) {
      int4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        v[u] = b0 + 4 * u < nblk ? *reinterpret_cast<const int4*>(row + b0 + 4 * u) : make_int4(0, 0, 0, 0);  // nblk_ld % 4 == 0
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = b0 + 4 * u;
        const int e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (b + q < nblk) {
            tot += (uint32_t)e[q];
            if (b + q < me) before += (uint32_t)e[q];
          }
      }
    }
  }
  // exclusive scan of tot over the digits: inside the wave, then over the waves
  uint32_t incl = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  {
    uint32_t off = 0;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    uint32_t running = off + incl - tot + before;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) {
      const uint32_t c = wbase[w][tid];
      wbase[w][tid] = running;
      running += c;
    }
  }
  __syncthreads();
  // 3. scatter: every wave on its own (LDS accesses of one wave execute in program order)
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const bool valid = (info[r] >> 16) & 1;
    const int d = (int)((key[r] >> shift) & (TS_RADIX - 1));
    const uint32_t rank = (uint32_t)(info[r] & 255), cnt = (uint32_t)((info[r] >> 8) & 255);
    const uint32_t b = valid ? mine_base[d] : 0u;
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) mine_base[d] = b + cnt;
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      if (kout) kout[b + rank] = key[r];
      pout[b + rank] = pl[r];
    }
  }
}

// offsets[r] = first sorted position whose key is >= r, r = 0 .. R (stored as the unsigned word: 2^31 at n = 2^31)
__global__ void __launch_bounds__(256)
ts_offsets_kernel(const uint32_t* __restrict__ sorted, int64_t n, int64_t R, int32_t* __restrict__ offsets) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= R; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)sorted[mid] < r) lo = mid + 1; else hi = mid;
    }
    offsets[r] = (int32_t)(uint32_t)lo;
  }
}

// digit passes of keys in [0, R): one per 9 bits of ceil(log2 R), at least one
int digit_passes(int64_t R) {
  int bits = 0;
  while (((int64_t)1 << bits) < R) ++bits;
  return std::max(1, (bits + TS_DIGIT_BITS - 1) / TS_DIGIT_BITS);
}

struct TablesWorkspace {
  size_t hist, key[2], pay[2], total;
  int nblk_ld;
};
TablesWorkspace tables_workspace(int64_t N) {
  TablesWorkspace w;
  const int64_t n = 2 * N;  // the node sort's keys; the relation sort (N keys) runs in the same buffers
  const int64_t nblk = ceil_div(n, TS_TILE);
  w.nblk_ld = (int)((nblk + 3) & ~(int64_t)3);
  auto take = [&w](size_t bytes) {
    const size_t off = w.total;
    w.total += (bytes + 255) & ~(size_t)255;
    return off;
  };
  w.total = 0;
  w.hist = take((size_t)TS_RADIX * w.nblk_ld * sizeof(int32_t));
  for (int i = 0; i < 2; ++i) w.key[i] = take((size_t)n * sizeof(uint32_t));
  for (int i = 0; i < 2; ++i) w.pay[i] = take((size_t)n * sizeof(uint32_t));
  return w;
}

// one table pair: entries = the positions 0 .. n - 1 stably sorted by key, offsets = row pointers of the R rows
int sort_pair(const int32_t* triples, int by_node, int64_t n, int64_t R, int32_t* offsets, int32_t* entries, char* ws,
              const TablesWorkspace& w, hipStream_t s) {
  const int passes = digit_passes(R);
  const int nblk = (int)ceil_div(n, TS_TILE);
  int32_t* hist = reinterpret_cast<int32_t*>(ws + w.hist);
  uint32_t* key[2] = {reinterpret_cast<uint32_t*>(ws + w.key[0]), reinterpret_cast<uint32_t*>(ws + w.key[1])};
  uint32_t* pay[2] = {reinterpret_cast<uint32_t*>(ws + w.pay[0]), reinterpret_cast<uint32_t*>(ws + w.pay[1])};
  for (int p = 0; p < passes; ++p) {
    const uint32_t* kin = p ? key[(p - 1) & 1] : nullptr;
    const uint32_t* pin = p ? pay[(p - 1) & 1] : nullptr;
    uint32_t* pout = p == passes - 1 ? reinterpret_cast<uint32_t*>(entries) : pay[p & 1];
    hipLaunchKernelGGL(ts_hist_kernel, dim3((unsigned)nblk), dim3(TS_THREADS), 0, s, kin, triples, by_node, n, p * TS_DIGIT_BITS,
                       hist, w.nblk_ld);
    TFGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_scatter_kernel, dim3((unsigned)nblk), dim3(TS_THREADS), 0, s, kin, pin, triples, by_node, n,
                       p * TS_DIGIT_BITS, (const int32_t*)hist, nblk, w.nblk_ld, key[p & 1], pout);
    TFGNN_LAUNCH_CHECK();
  }
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(R + 1, 256), 8192));
  hipLaunchKernelGGL(ts_offsets_kernel, dim3(blocks), dim3(256), 0, s, (const uint32_t*)key[(passes - 1) & 1], n, R, offsets);
  TFGNN_LAUNCH_CHECK();
  g_negatives_launches[1].fetch_add(2 * passes + 1, std::memory_order_relaxed);
  return TFGNN_OK;
}

}  // namespace
}  // namespace tfgnn

using namespace tfgnn;

extern "C" int tfgnn_triples_draw_negatives(int32_t* d_triples, int64_t N, int64_t P, int64_t K, int64_t V, uint64_t seed,
                                            int use_epoch, void* stream) {
  TFGNN_REQUIRE(P >= 1, "triples_draw_negatives: empty batch (no positive)");
  TFGNN_REQUIRE(N >= 1 && N <= ((int64_t)1 << 30), "triples_draw_negatives: N must be in [1, 2^30]");
  TFGNN_REQUIRE(K >= 0 && K < N && P <= N && N == P * (1 + K), "triples_draw_negatives: N must be P (1 + K), K >= 0");
  TFGNN_REQUIRE(d_triples, "triples_draw_negatives: NULL pointer");
  TFGNN_REQUIRE(V >= 1 && V < ((int64_t)1 << 31), "triples_draw_negatives: V must be in [1, 2^31)");
  TFGNN_REQUIRE(K == 0 || V >= 2, "triples_draw_negatives: a negative needs a second node (V >= 2)");
  if (K == 0) return TFGNN_OK;
  DropoutKey key = dropout_key(seed, 0.f);  // the key words alone: no threshold, no scale
  key.epoch = nullptr;
  if (use_epoch) {
    key.epoch = dropout_epoch_word();
    TFGNN_REQUIRE(key.epoch, "triples_draw_negatives: no device memory for the epoch word");
  }
  const int64_t negatives = P * K;
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(negatives, DRAW_THREADS), 8192);
  hipLaunchKernelGGL(draw_negatives_kernel, dim3(blocks), dim3(DRAW_THREADS), 0, (hipStream_t)stream, d_triples, P, (uint32_t)K,
                     negatives, (uint32_t)(V - 1), key);
  TFGNN_LAUNCH_CHECK();
  g_negatives_launches[0].fetch_add(1, std::memory_order_relaxed);
  return TFGNN_OK;
}

extern "C" size_t tfgnn_triple_tables_workspace_bytes(int64_t N, int64_t V, int64_t T) {
  if (N < 1 || N > ((int64_t)1 << 30) || V < 1 || T < 1) return 0;
  return tables_workspace(N).total;
}

extern "C" int tfgnn_triple_tables_build(const int32_t* d_triples, int64_t N, int64_t V, int64_t T, int32_t* d_node_offsets,
                                         int32_t* d_node_entries, int32_t* d_rel_offsets, int32_t* d_rel_order, void* d_workspace,
                                         size_t workspace_bytes, void* stream) {
  TFGNN_REQUIRE(N >= 1, "triple_tables_build: empty batch (no triple)");
  TFGNN_REQUIRE(N <= ((int64_t)1 << 30), "triple_tables_build: more than 2^30 triples");
  TFGNN_REQUIRE(V >= 1 && V < ((int64_t)1 << 31) && T >= 1 && T < ((int64_t)1 << 31), "triple_tables_build: V and T must be in [1, 2^31)");
  TFGNN_REQUIRE(d_triples, "triple_tables_build: NULL pointer");
  TFGNN_REQUIRE((d_node_offsets == nullptr) == (d_node_entries == nullptr) && (d_rel_offsets == nullptr) == (d_rel_order == nullptr),
                "triple_tables_build: the tables come in pairs (offsets with entries, offsets with order)");
  TFGNN_REQUIRE(d_node_offsets || d_rel_offsets, "triple_tables_build: NULL pointer (no table requested)");
  const TablesWorkspace w = tables_workspace(N);
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= w.total && (uintptr_t)d_workspace % 16 == 0,
                "triple_tables_build: workspace too small or misaligned (need %zu bytes, 16-byte aligned)", w.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(d_workspace);
  if (d_node_offsets) {
    const int rc = sort_pair(d_triples, 1, 2 * N, V, d_node_offsets, d_node_entries, ws, w, s);
    if (rc) return rc;
  }
  if (d_rel_offsets) {
    const int rc = sort_pair(d_triples, 0, N, T, d_rel_offsets, d_rel_order, ws, w, s);
    if (rc) return rc;
  }
  return TFGNN_OK;
}

extern "C" int tfgnn_negatives_launch_counts(int64_t* out_counts, int n) {
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_negatives_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i < 2 ? g_negatives_launches[i].load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}
