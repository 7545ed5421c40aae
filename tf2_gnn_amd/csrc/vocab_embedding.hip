// Vocabulary embeddings: a row lookup whose ids REPEAT, and its table gradient - a segment sum of d_rows over equal ids
// (include/tfgnn.h "Vocabulary embeddings" has the contract and the order of the sums).
//
// Forward, 2 + 2 * passes launches: the lookup (one thread per row validates the id and leaves the sort key - the id, or N for
// an invalid one - in the workspace; then the workgroup copies the tile's rows, consecutive lanes on consecutive floats, as
// embedding.hip does), a stable LSD radix sort of (key, row index) and the row pointers.  The sort is the scheme of
// negatives.hip, in a copy of its own (that file's compiled code is pinned by tests): 9-bit digits, 8192 keys per workgroup,
// per-tile digit histograms in a [digit][tile] table, a wave ranks its 1024 consecutive keys with ballots.  No global atomic.
//
// Backward, 1 or 2 launches.  The sorted positions of id r are [off[r], off[r + 1]); its chunk k is the positions
// [off[r] + 256 k, min(off[r] + 256 (k + 1), off[r + 1])).  No chunk table is stored and nothing is scanned, because the chunks
// can be found from the row pointers alone:
//   - chunk 0 of id r belongs to work item r (N items).  The same item writes the zeros of an absent id.
//   - a chunk k >= 1 starts 256 positions after another chunk of its id, so an aligned block [256 b, 256 b + 256) of sorted
//     positions holds at most one such start, and it belongs to the id that sits on position 256 b.  Work item N + b looks for it.
// One wave takes one (work item, slab of 256 columns): the lanes stage the chunk's <= 256 row indices in LDS (four coalesced
// loads, each checked against n), then every lane walks the rows with its own float4 column group (scalar path: four columns
// 64 apart), eight row loads in flight ahead of the adds.  An id of one chunk is stored straight to table_grad.  A chunk of a
// longer id goes to partial row 2 * (start / 256) + (k == 0): chunk 0 of such an id is full, so no two of them start in one
// block, and the k >= 1 start of a block is unique - the slots do not collide and there are 2 * ceil(n / 256) of them.  The
// second launch has one wave per block and slab: the wave whose block holds chunk 1 of an id adds that id's partials in
// chunk order and stores the row.  Plain stores only; no float atomics; the grids come from n, N and D.
#include <atomic>

#include "common.hpp"

namespace tfgnn {
namespace {

std::atomic<int64_t> g_vocab_launches[2];  // forward, backward

// ---- the lookup -----------------------------------------------------------------------------------------------------------
constexpr int VL_THREADS = 256;
constexpr int VL_TILE_ELEMS = 8192;  // floats one workgroup copies unless a single row is longer

struct LookupParams {
  const float* table;  // [N, D], pitch ld_table
  const int32_t* ids_i;
  const float* ids_f;
  float* out;      // [n, D], pitch ld_out
  uint32_t* keys;  // [n]: the id, N for an invalid one
  int* bad;
  int64_t ld_table, ld_out, ids_pitch;
  int32_t n, N, D;
  int rows_per_tile, vec4;
};

__global__ void __launch_bounds__(VL_THREADS) vocab_lookup_kernel(const LookupParams P) {
  __shared__ int32_t src_rows[VL_THREADS];
  const int64_t r0 = (int64_t)blockIdx.x * P.rows_per_tile;
  const int rows = (int)min((int64_t)P.rows_per_tile, (int64_t)P.n - r0);
  for (int i = threadIdx.x; i < rows; i += VL_THREADS) {
    const int64_t idx = r0 + i;
    int32_t id;
    bool ok;
    if (P.ids_i) {
      id = P.ids_i[idx * P.ids_pitch];
      ok = (uint32_t)id < (uint32_t)P.N;
    } else {
      const float f = P.ids_f[idx * P.ids_pitch];  // N <= 2^24: (float)N is exact.  NaN fails the first test, -0.0 is id 0
      ok = f >= 0.f && f < (float)P.N && f == floorf(f);
      id = ok ? (int32_t)f : -1;
    }
    if (!ok) {
      id = -1;
      if (P.bad) *P.bad = 1;
    }
    src_rows[i] = id;
    P.keys[idx] = ok ? (uint32_t)id : (uint32_t)P.N;
  }
  __syncthreads();
  if (P.vec4) {
    const uint32_t F4 = (uint32_t)P.D >> 2;
    const uint32_t cnt = (uint32_t)rows * F4;
    const int64_t ld_in = P.ld_table >> 2, ld_o = P.ld_out >> 2;
    const float4* __restrict__ in = reinterpret_cast<const float4*>(P.table);
    float4* __restrict__ out = reinterpret_cast<float4*>(P.out) + r0 * ld_o;
    for (uint32_t e = threadIdx.x; e < cnt; e += VL_THREADS) {
      const uint32_t row = e / F4, c = e - row * F4;
      const int32_t s = src_rows[row];
      out[(int64_t)row * ld_o + c] = s >= 0 ? in[(int64_t)s * ld_in + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  } else {
    const uint32_t F = (uint32_t)P.D;
    const uint32_t cnt = (uint32_t)rows * F;
    const float* __restrict__ in = P.table;
    float* __restrict__ out = P.out + r0 * P.ld_out;
    for (uint32_t e = threadIdx.x; e < cnt; e += VL_THREADS) {
      const uint32_t row = e / F, c = e - row * F;
      const int32_t s = src_rows[row];
      out[(int64_t)row * P.ld_out + c] = s >= 0 ? in[(int64_t)s * P.ld_table + c] : 0.f;
    }
  }
}

// ---- the plan: stable LSD radix sort of 32-bit keys with the row index as payload ----------------------------------------------
constexpr int VS_THREADS = 512;
constexpr int VS_ROUNDS = 16;
constexpr int VS_WAVES = VS_THREADS / 64;
constexpr int VS_WAVE_KEYS = 64 * VS_ROUNDS;     // consecutive keys per wave
constexpr int VS_TILE = VS_THREADS * VS_ROUNDS;  // 8192 keys per workgroup
constexpr int VS_DIGIT_BITS = 9;
constexpr int VS_RADIX = 1 << VS_DIGIT_BITS;     // 512 = one digit per thread
static_assert(VS_RADIX == VS_THREADS, "one digit per thread");

// hist[digit * nblk_ld + tile] = number of keys of the tile with that digit
__global__ void __launch_bounds__(VS_THREADS)
vocab_sort_hist_kernel(const uint32_t* __restrict__ kin, int64_t n, int shift, int32_t* __restrict__ hist, int nblk_ld) {
  __shared__ int32_t h[VS_RADIX];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * VS_TILE;
#pragma unroll 4
  for (int r = 0; r < VS_ROUNDS; ++r) {
    const int64_t idx = base + r * VS_THREADS + tid;
    if (idx < n) atomicAdd(&h[(int)((kin[idx] >> shift) & (VS_RADIX - 1))], 1);  // LDS; a count: any order
  }
  __syncthreads();
  hist[(int64_t)tid * nblk_ld + blockIdx.x] = h[tid];
}

// stable scatter of one digit: keys keep their input order inside a digit (tile, then wave, round, lane = index order).
// pin == NULL (first pass): the payload is the key's index
__global__ void __launch_bounds__(VS_THREADS)
vocab_sort_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ pin, int64_t n, int shift,
                          const int32_t* __restrict__ hist, int nblk, int nblk_ld, uint32_t* __restrict__ kout,
                          uint32_t* __restrict__ pout) {
  __shared__ uint32_t wbase[VS_WAVES][VS_RADIX];  // per wave: digit counts, then running output positions
  __shared__ uint32_t wtot[VS_WAVES];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  volatile uint32_t* mine_base = &wbase[wave][0];
#pragma unroll
  for (int i = 0; i < VS_RADIX / 64; ++i) mine_base[lane + 64 * i] = 0;
  __builtin_amdgcn_wave_barrier();
  // 1. keys into registers; digit counts of this wave (one leader lane per digit and round adds the group size)
  const int64_t wave0 = (int64_t)blockIdx.x * VS_TILE + (int64_t)wave * VS_WAVE_KEYS;
  const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  uint32_t key[VS_ROUNDS], pl[VS_ROUNDS];
  int32_t info[VS_ROUNDS];  // rank | group size << 8 | valid << 16
#pragma unroll
  for (int r = 0; r < VS_ROUNDS; ++r) {
    const int64_t idx = wave0 + r * 64 + lane;
    const bool valid = idx < n;
    key[r] = valid ? kin[idx] : 0u;
    pl[r] = valid ? (pin ? pin[idx] : (uint32_t)idx) : 0u;
  }
#pragma unroll
  for (int r = 0; r < VS_ROUNDS; ++r) {
    const bool valid = wave0 + r * 64 + lane < n;
    const int d = (int)((key[r] >> shift) & (VS_RADIX - 1));
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < VS_DIGIT_BITS; ++b) {
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
  uint32_t tot = 0, before = 0;
  {
    const int32_t* __restrict__ row = hist + (int64_t)tid * nblk_ld;
    const int me = (int)blockIdx.x;
    for (int b0 = 0; b0 < nblk; b0 += 4) {
      const int4 v = *reinterpret_cast<const int4*>(row + b0);  // nblk_ld % 4 == 0; the pad columns are never summed
      const int e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (b0 + q < nblk) {
          tot += (uint32_t)e[q];
          if (b0 + q < me) before += (uint32_t)e[q];
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
    for (int w = 0; w < VS_WAVES; ++w) {
      const uint32_t c = wbase[w][tid];
      wbase[w][tid] = running;
      running += c;
    }
  }
  __syncthreads();
  // 3. scatter: every wave on its own (LDS accesses of one wave execute in program order).  The positions are below n by
  //    construction - the histograms count exactly the n keys -; the comparison keeps a wrong table from writing outside
#pragma unroll
  for (int r = 0; r < VS_ROUNDS; ++r) {
    const bool valid = (info[r] >> 16) & 1;
    const int d = (int)((key[r] >> shift) & (VS_RADIX - 1));
    const uint32_t rank = (uint32_t)(info[r] & 255), cnt = (uint32_t)((info[r] >> 8) & 255);
    const uint32_t b = valid ? mine_base[d] : 0u;
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) mine_base[d] = b + cnt;
    __builtin_amdgcn_wave_barrier();
    if (valid && (int64_t)(b + rank) < n) {
      kout[b + rank] = key[r];
      pout[b + rank] = pl[r];
    }
  }
}

// offsets[r] = first sorted position whose key is >= r, r = 0 .. N; offsets[N] is the number of valid rows
__global__ void __launch_bounds__(256)
vocab_offsets_kernel(const uint32_t* __restrict__ sorted, int64_t n, int64_t N, int32_t* __restrict__ offsets) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= N; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)sorted[mid] < r) lo = mid + 1; else hi = mid;
    }
    offsets[r] = (int32_t)lo;
  }
}

// digit passes of keys in [0, N]: one per 9 bits of bit_length(N), at least one
int digit_passes(int64_t N) {
  int bits = 0;
  while (((int64_t)1 << bits) <= N) ++bits;
  return std::max(1, (bits + VS_DIGIT_BITS - 1) / VS_DIGIT_BITS);
}

// the plan in the caller's workspace; a function of (n, N) alone, so the backward call finds what the forward call left
struct PlanLayout {
  size_t hist, key[2], pay[2], offsets, total;
  int nblk, nblk_ld, passes;
  int sorted;  // which of key[] / pay[] holds the result
};
PlanLayout plan_layout(int64_t n, int64_t N) {
  PlanLayout w;
  w.nblk = (int)ceil_div(n, VS_TILE);
  w.nblk_ld = (w.nblk + 3) & ~3;
  w.passes = digit_passes(N);
  w.sorted = (w.passes - 1) & 1;
  w.total = 0;
  auto take = [&w](size_t bytes) {
    const size_t off = w.total;
    w.total += (bytes + 255) & ~(size_t)255;
    return off;
  };
  w.hist = take((size_t)VS_RADIX * w.nblk_ld * sizeof(int32_t));
  for (int i = 0; i < 2; ++i) w.key[i] = take((size_t)n * sizeof(uint32_t));
  for (int i = 0; i < 2; ++i) w.pay[i] = take((size_t)n * sizeof(uint32_t));
  w.offsets = take((size_t)(N + 1) * sizeof(int32_t));
  return w;
}

// ---- the reduce -----------------------------------------------------------------------------------------------------------
constexpr int VR_THREADS = 256;
constexpr int VR_WAVES = VR_THREADS / 64;
constexpr int VR_CHUNK = 256;   // sorted positions per chunk
constexpr int VR_SLAB = 256;    // columns per wave
constexpr int VR_FLIGHT = 8;    // row loads in flight

struct ReduceParams {
  const float* rows;        // d_rows [n, D], pitch ld_rows
  const uint32_t* keys;     // sorted keys [n]
  const uint32_t* order;    // sorted row indices [n]
  const int32_t* offsets;   // [N + 1]; NULL when n == 0: every id is absent
  float* partials;          // [partial_rows, D] contiguous
  float* grad;              // [N, D], pitch ld_grad
  int64_t ld_rows, ld_grad, partial_rows;
  int32_t n, N, D;
  int64_t nblocks;          // ceil(n / 256)
};

// the lane's four floats of row `base`: one float4 (columns 4 c4 ..) or the columns c4 + 64 j of the slab
template <bool VEC>
__device__ __forceinline__ float4 load_cols(const float* __restrict__ base, int col, int D) {
  if (VEC) return col < D ? *reinterpret_cast<const float4*>(base + col) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v;
  v.x = col < D ? base[col] : 0.f;
  v.y = col + 64 < D ? base[col + 64] : 0.f;
  v.z = col + 128 < D ? base[col + 128] : 0.f;
  v.w = col + 192 < D ? base[col + 192] : 0.f;
  return v;
}
template <bool VEC>
__device__ __forceinline__ void store_cols(float* __restrict__ base, int col, int D, const float4 v) {
  if (VEC) {
    if (col < D) *reinterpret_cast<float4*>(base + col) = v;
    return;
  }
  if (col < D) base[col] = v.x;
  if (col + 64 < D) base[col + 64] = v.y;
  if (col + 128 < D) base[col + 128] = v.z;
  if (col + 192 < D) base[col + 192] = v.w;
}
__device__ __forceinline__ void add4(float4& a, const float4 b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// row pointers of id r, clamped so that a damaged plan cannot send a read past n
__device__ __forceinline__ void segment_of(const ReduceParams& P, int32_t r, int64_t& s, int64_t& e) {
  s = min(max((int64_t)P.offsets[r], (int64_t)0), (int64_t)P.n);
  e = min(max((int64_t)P.offsets[r + 1], s), (int64_t)P.n);
}
// the chunk k >= 1 that starts inside block b, if any: its id, k and start
__device__ __forceinline__ bool later_chunk_of_block(const ReduceParams& P, int64_t b, int32_t& id, int64_t& s, int64_t& e,
                                                     int64_t& start) {
  const int64_t first = b * VR_CHUNK;
  if (first >= P.n) return false;
  const uint32_t key = P.keys[first];
  if (key >= (uint32_t)P.N) return false;  // the invalid rows: sorted last, in nobody's sum
  id = (int32_t)key;
  segment_of(P, id, s, e);
  if (s >= first) return false;  // the id starts here: chunk 0, work item `id`
  start = s + (first - s + VR_CHUNK - 1) / VR_CHUNK * VR_CHUNK;
  return start < e;
}

template <bool VEC>
__global__ void __launch_bounds__(VR_THREADS) vocab_reduce_kernel(const ReduceParams P) {
  __shared__ int32_t staged[VR_WAVES][VR_CHUNK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t item = (int64_t)blockIdx.x * VR_WAVES + wave;
  const int col = (int)blockIdx.y * VR_SLAB + (VEC ? 4 * lane : lane);
  int32_t id = -1;
  int64_t start = 0, len = 0;
  bool whole = true;  // the chunk is all of its id: straight to table_grad
  if (item < P.N) {
    id = (int32_t)item;
    if (P.offsets) {
      int64_t s, e;
      segment_of(P, id, s, e);
      start = s;
      len = min(e - s, (int64_t)VR_CHUNK);
      whole = e - s <= VR_CHUNK;
    }
  } else if (item - P.N < P.nblocks) {
    int64_t s, e;
    if (later_chunk_of_block(P, item - P.N, id, s, e, start)) {
      len = min(e - start, (int64_t)VR_CHUNK);
      whole = false;
    } else {
      id = -1;
    }
  }
  // the chunk's row indices, once: four coalesced loads per wave, each index checked against n (-1: not read)
  int32_t* mine = staged[wave];
#pragma unroll
  for (int j = 0; j < VR_CHUNK / 64; ++j) {
    const int q = lane + 64 * j;
    int32_t r = -1;
    if (q < len) {
      const uint32_t v = P.order[start + q];
      if (v < (uint32_t)P.n) r = (int32_t)v;
    }
    mine[q] = r;
  }
  __syncthreads();
  if (id < 0) return;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  bool have = false;  // the first row is taken as it is: a single row keeps its bits, -0.0 included
  const int count = (int)len;
  for (int i = 0; i < count; i += VR_FLIGHT) {
    float4 v[VR_FLIGHT];
    int32_t r[VR_FLIGHT];
#pragma unroll
    for (int u = 0; u < VR_FLIGHT; ++u) {
      r[u] = i + u < count ? __builtin_amdgcn_readfirstlane(mine[i + u]) : -1;
      if (r[u] >= 0) v[u] = load_cols<VEC>(P.rows + (int64_t)r[u] * P.ld_rows, col, P.D);
    }
#pragma unroll
    for (int u = 0; u < VR_FLIGHT; ++u) {
      if (r[u] < 0) continue;
      if (have) add4(acc, v[u]); else acc = v[u];
      have = true;
    }
  }
  if (whole) {
    store_cols<VEC>(P.grad + (int64_t)id * P.ld_grad, col, P.D, acc);
  } else {
    const int64_t slot = 2 * (start / VR_CHUNK) + (item < P.N ? 1 : 0);
    if (slot < P.partial_rows) store_cols<VEC>(P.partials + slot * P.D, col, P.D, acc);
  }
}

// one wave per (block, slab): the wave whose block holds chunk 1 of an id adds the id's partials, chunk 0 first
template <bool VEC>
__global__ void __launch_bounds__(VR_THREADS) vocab_combine_kernel(const ReduceParams P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * VR_WAVES + wave;
  const int col = (int)blockIdx.y * VR_SLAB + (VEC ? 4 * lane : lane);
  if (b >= P.nblocks) return;
  int32_t id;
  int64_t s, e, start;
  if (!later_chunk_of_block(P, b, id, s, e, start) || start != s + VR_CHUNK) return;
  const int64_t chunks = (e - s + VR_CHUNK - 1) / VR_CHUNK;  // >= 2
  const int64_t slot0 = 2 * (s / VR_CHUNK) + 1;
  float4 acc = slot0 < P.partial_rows ? load_cols<VEC>(P.partials + slot0 * P.D, col, P.D) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t k = 1; k < chunks; k += VR_FLIGHT) {
    float4 v[VR_FLIGHT];
#pragma unroll
    for (int u = 0; u < VR_FLIGHT; ++u) {
      const int64_t slot = 2 * ((s + (k + u) * VR_CHUNK) / VR_CHUNK);
      if (k + u < chunks && slot < P.partial_rows) v[u] = load_cols<VEC>(P.partials + slot * P.D, col, P.D);
    }
#pragma unroll
    for (int u = 0; u < VR_FLIGHT; ++u) {
      const int64_t slot = 2 * ((s + (k + u) * VR_CHUNK) / VR_CHUNK);
      if (k + u < chunks && slot < P.partial_rows) add4(acc, v[u]);
    }
  }
  store_cols<VEC>(P.grad + (int64_t)id * P.ld_grad, col, P.D, acc);
}

constexpr int64_t kLimit = (int64_t)1 << 31;
constexpr int64_t kMaxSlabs = 65535;  // grid y

}  // namespace
}  // namespace tfgnn

using namespace tfgnn;

extern "C" size_t tfgnn_vocab_embedding_workspace_bytes(int64_t n, int64_t N) {
  if (n < 0 || n >= kLimit || N < 1 || N >= kLimit) return 0;
  return plan_layout(n, N).total;
}

extern "C" int tfgnn_vocab_embedding_forward(const tfgnn_vocab_embedding_forward_args* a, void* stream) {
  TFGNN_REQUIRE(a && a->struct_size == sizeof(*a), "vocab_embedding_forward: NULL args or a struct of another size");
  const int64_t n = a->n, N = a->N, D = a->D;
  TFGNN_REQUIRE(n >= 0 && N >= 0, "vocab_embedding_forward: negative size");
  TFGNN_REQUIRE(n < kLimit && N < kLimit, "vocab_embedding_forward: 2^31 or more rows or ids");
  TFGNN_REQUIRE(D >= 1 && D < kLimit, "vocab_embedding_forward: D must be in [1, 2^31)");
  TFGNN_REQUIRE(n == 0 || N >= 1, "vocab_embedding_forward: rows to look up in an empty vocabulary (N == 0)");
  if (n == 0) return TFGNN_OK;
  TFGNN_REQUIRE(a->ld_table >= D && a->ld_out >= D, "vocab_embedding_forward: a row pitch below D");
  TFGNN_REQUIRE((a->ids_i32 == nullptr) != (a->ids_f32 == nullptr), "vocab_embedding_forward: exactly one of ids_i32 and ids_f32");
  TFGNN_REQUIRE(a->ids_pitch >= 1, "vocab_embedding_forward: ids_pitch must be at least 1");
  TFGNN_REQUIRE(!a->ids_f32 || N <= ((int64_t)1 << 24), "vocab_embedding_forward: float ids need N <= 2^24");
  TFGNN_REQUIRE(a->table && a->out, "vocab_embedding_forward: NULL table or out");
  const PlanLayout w = plan_layout(n, N);
  TFGNN_REQUIRE(a->workspace && a->workspace_bytes >= w.total && (uintptr_t)a->workspace % 16 == 0,
                "vocab_embedding_forward: workspace too small or misaligned (need %zu bytes, 16-byte aligned)", w.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(a->workspace);
  int32_t* hist = reinterpret_cast<int32_t*>(ws + w.hist);
  uint32_t* key[2] = {reinterpret_cast<uint32_t*>(ws + w.key[0]), reinterpret_cast<uint32_t*>(ws + w.key[1])};
  uint32_t* pay[2] = {reinterpret_cast<uint32_t*>(ws + w.pay[0]), reinterpret_cast<uint32_t*>(ws + w.pay[1])};

  LookupParams P;
  memset(&P, 0, sizeof(P));
  P.table = a->table;
  P.ids_i = a->ids_i32;
  P.ids_f = a->ids_f32;
  P.out = a->out;
  P.keys = key[1];  // pass p reads key[(p + 1) & 1] and writes key[p & 1]
  P.bad = a->bad_flag;
  P.ld_table = a->ld_table;
  P.ld_out = a->ld_out;
  P.ids_pitch = a->ids_pitch;
  P.n = (int32_t)n;
  P.N = (int32_t)N;
  P.D = (int32_t)D;
  P.rows_per_tile = (int)std::max<int64_t>(1, std::min<int64_t>(VL_THREADS, VL_TILE_ELEMS / D));
  P.vec4 = D % 4 == 0 && a->ld_table % 4 == 0 && a->ld_out % 4 == 0 && (uintptr_t)a->table % 16 == 0 && (uintptr_t)a->out % 16 == 0;
  hipLaunchKernelGGL(vocab_lookup_kernel, dim3((unsigned)ceil_div(n, P.rows_per_tile)), dim3(VL_THREADS), 0, s, P);
  TFGNN_LAUNCH_CHECK();
  for (int p = 0; p < w.passes; ++p) {
    const uint32_t* kin = key[(p + 1) & 1];
    const uint32_t* pin = p ? pay[(p + 1) & 1] : nullptr;
    hipLaunchKernelGGL(vocab_sort_hist_kernel, dim3((unsigned)w.nblk), dim3(VS_THREADS), 0, s, kin, n, p * VS_DIGIT_BITS, hist,
                       w.nblk_ld);
    TFGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(vocab_sort_scatter_kernel, dim3((unsigned)w.nblk), dim3(VS_THREADS), 0, s, kin, pin, n, p * VS_DIGIT_BITS,
                       (const int32_t*)hist, w.nblk, w.nblk_ld, key[p & 1], pay[p & 1]);
    TFGNN_LAUNCH_CHECK();
  }
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(N + 1, 256), 8192));
  hipLaunchKernelGGL(vocab_offsets_kernel, dim3(blocks), dim3(256), 0, s, (const uint32_t*)key[w.sorted], n, N,
                     reinterpret_cast<int32_t*>(ws + w.offsets));
  TFGNN_LAUNCH_CHECK();
  g_vocab_launches[0].fetch_add(2 + 2 * w.passes, std::memory_order_relaxed);
  return TFGNN_OK;
}

extern "C" int tfgnn_vocab_embedding_backward(const tfgnn_vocab_embedding_backward_args* a, void* stream) {
  TFGNN_REQUIRE(a && a->struct_size == sizeof(*a), "vocab_embedding_backward: NULL args or a struct of another size");
  const int64_t n = a->n, N = a->N, D = a->D;
  TFGNN_REQUIRE(n >= 0 && N >= 0, "vocab_embedding_backward: negative size");
  TFGNN_REQUIRE(n < kLimit && N < kLimit, "vocab_embedding_backward: 2^31 or more rows or ids");
  TFGNN_REQUIRE(D >= 1 && D < kLimit, "vocab_embedding_backward: D must be in [1, 2^31)");
  TFGNN_REQUIRE(n == 0 || N >= 1, "vocab_embedding_backward: rows of an empty vocabulary (N == 0)");
  if (N == 0) return TFGNN_OK;
  const int64_t slabs = ceil_div(D, VR_SLAB);
  if (slabs > kMaxSlabs) {
    set_error("vocab_embedding_backward: D above %lld columns (65535 slabs of 256)", (long long)(kMaxSlabs * VR_SLAB));
    return TFGNN_ERR_UNSUPPORTED;
  }
  TFGNN_REQUIRE(a->table_grad && a->ld_grad >= D, "vocab_embedding_backward: NULL table_grad or a pitch below D");
  ReduceParams P;
  memset(&P, 0, sizeof(P));
  P.grad = a->table_grad;
  P.ld_grad = a->ld_grad;
  P.n = (int32_t)n;
  P.N = (int32_t)N;
  P.D = (int32_t)D;
  P.nblocks = ceil_div(n, VR_CHUNK);
  bool vec = D % 4 == 0 && a->ld_grad % 4 == 0 && (uintptr_t)a->table_grad % 16 == 0;
  if (n > 0) {
    TFGNN_REQUIRE(a->d_rows && a->ld_rows >= D, "vocab_embedding_backward: NULL d_rows or a pitch below D");
    const PlanLayout w = plan_layout(n, N);
    TFGNN_REQUIRE(a->workspace && a->workspace_bytes >= w.total && (uintptr_t)a->workspace % 16 == 0,
                  "vocab_embedding_backward: plan workspace too small or misaligned (need %zu bytes, 16-byte aligned)", w.total);
    const char* ws = static_cast<const char*>(a->workspace);
    P.rows = a->d_rows;
    P.ld_rows = a->ld_rows;
    P.keys = reinterpret_cast<const uint32_t*>(ws + w.key[w.sorted]);
    P.order = reinterpret_cast<const uint32_t*>(ws + w.pay[w.sorted]);
    P.offsets = reinterpret_cast<const int32_t*>(ws + w.offsets);
    vec = vec && a->ld_rows % 4 == 0 && (uintptr_t)a->d_rows % 16 == 0;
    if (n > VR_CHUNK) {  // an id of several chunks is possible
      P.partial_rows = TFGNN_VOCAB_EMBEDDING_PARTIAL_ROWS(n);
      const size_t need = (size_t)P.partial_rows * (size_t)D * sizeof(float);
      TFGNN_REQUIRE(a->partials && a->partials_bytes >= need && (uintptr_t)a->partials % 16 == 0,
                    "vocab_embedding_backward: partials too small or misaligned (need %zu bytes, 16-byte aligned)", need);
      P.partials = a->partials;
    }
  }
  const int64_t items = N + P.nblocks;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(items, VR_WAVES), (unsigned)slabs);
  if (vec) hipLaunchKernelGGL(vocab_reduce_kernel<true>, grid, dim3(VR_THREADS), 0, s, P);
  else hipLaunchKernelGGL(vocab_reduce_kernel<false>, grid, dim3(VR_THREADS), 0, s, P);
  TFGNN_LAUNCH_CHECK();
  int launches = 1;
  if (n > VR_CHUNK) {
    const dim3 grid2((unsigned)ceil_div(P.nblocks, VR_WAVES), (unsigned)slabs);
    if (vec) hipLaunchKernelGGL(vocab_combine_kernel<true>, grid2, dim3(VR_THREADS), 0, s, P);
    else hipLaunchKernelGGL(vocab_combine_kernel<false>, grid2, dim3(VR_THREADS), 0, s, P);
    TFGNN_LAUNCH_CHECK();
    ++launches;
  }
  g_vocab_launches[1].fetch_add(launches, std::memory_order_relaxed);
  return TFGNN_OK;
}

extern "C" int tfgnn_vocab_embedding_launch_counts(int64_t* out_counts, int n) {
  TFGNN_REQUIRE(out_counts && n >= 0, "tfgnn_vocab_embedding_launch_counts: bad argument");
  for (int i = 0; i < n; ++i) out_counts[i] = i < 2 ? g_vocab_launches[i].load(std::memory_order_relaxed) : 0;
  return TFGNN_OK;
}
