// Gradient of an embedding lookup with distinct ids, as a dense table gradient (include/tfgnn.h "Node embeddings").
//
// Two launches per call, on one stream, in this order:
//   fill      every element [r, 0:D) of table_grad becomes 0.  kEmbTileElems floats to a workgroup (whole rows, one row when
//             a row is longer), consecutive lanes on consecutive floats of a row.
//   scatter   rows_per_tile rows of `rows` to a workgroup.  One thread per row reads the row's id, checks it against N and
//             leaves it in LDS (-1: skipped, *bad set); then the whole workgroup copies the tile's rows_per_tile * D floats,
//             consecutive lanes on consecutive floats of the source and of the destination row.
// float4 in both when D % 4 == 0, both buffers are 16-byte aligned and both pitches are multiples of 4.  The ids are distinct
// by precondition, so no two workgroups write the same row: plain stores, no atomics.  Every write is to a row < N and a
// column < D; every read of `rows` and `ids` is below n.
#include <atomic>

#include "common.hpp"

namespace tfgnn {

constexpr int kEmbThreads = 256;
constexpr int kEmbTileElems = 8192;  // floats one workgroup writes (32 per thread) unless a single row is longer

static std::atomic<int64_t> g_embedding_launches;

struct EmbParams {
  const float* rows;   // [n, D], pitch ld_rows
  const int32_t* ids;  // [n]
  float* grad;         // [N, D], pitch ld_grad
  int64_t ld_rows, ld_grad;
  int32_t n, N, D;
  int rows_per_tile, vec4;
  int* bad;
};

__global__ void __launch_bounds__(kEmbThreads) embedding_fill_kernel(const EmbParams P) {
  const int64_t r0 = (int64_t)blockIdx.x * P.rows_per_tile;
  const int rows = (int)min((int64_t)P.rows_per_tile, (int64_t)P.N - r0);
  if (P.vec4) {
    const uint32_t F4 = (uint32_t)P.D >> 2;
    const uint32_t cnt = (uint32_t)rows * F4;
    const int64_t ld4 = P.ld_grad >> 2;
    float4* __restrict__ out = reinterpret_cast<float4*>(P.grad) + r0 * ld4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t e = threadIdx.x; e < cnt; e += kEmbThreads) {
      const uint32_t row = e / F4, c = e - row * F4;
      out[(int64_t)row * ld4 + c] = zero;
    }
  } else {
    const uint32_t F = (uint32_t)P.D;
    const uint32_t cnt = (uint32_t)rows * F;
    float* __restrict__ out = P.grad + r0 * P.ld_grad;
    for (uint32_t e = threadIdx.x; e < cnt; e += kEmbThreads) {
      const uint32_t row = e / F, c = e - row * F;
      out[(int64_t)row * P.ld_grad + c] = 0.f;
    }
  }
}

__global__ void __launch_bounds__(kEmbThreads) embedding_scatter_kernel(const EmbParams P) {
  __shared__ int32_t dst_rows[kEmbThreads];
  const int32_t r0 = (int32_t)blockIdx.x * P.rows_per_tile;  // < n <= N < 2^31
  const int rows = min(P.rows_per_tile, P.n - r0);
  for (int i = threadIdx.x; i < rows; i += kEmbThreads) {
    int32_t id = P.ids[r0 + i];
    if ((uint32_t)id >= (uint32_t)P.N) {
      id = -1;
      if (P.bad) *P.bad = 1;
    }
    dst_rows[i] = id;
  }
  __syncthreads();
  if (P.vec4) {
    const uint32_t F4 = (uint32_t)P.D >> 2;
    const uint32_t cnt = (uint32_t)rows * F4;
    const int64_t ld_in = P.ld_rows >> 2, ld_out = P.ld_grad >> 2;
    const float4* __restrict__ in = reinterpret_cast<const float4*>(P.rows) + (int64_t)r0 * ld_in;
    float4* __restrict__ out = reinterpret_cast<float4*>(P.grad);
    for (uint32_t e = threadIdx.x; e < cnt; e += kEmbThreads) {
      const uint32_t row = e / F4, c = e - row * F4;
      const int32_t d = dst_rows[row];
      if (d >= 0) out[(int64_t)d * ld_out + c] = in[(int64_t)row * ld_in + c];
    }
  } else {
    const uint32_t F = (uint32_t)P.D;
    const uint32_t cnt = (uint32_t)rows * F;
    const float* __restrict__ in = P.rows + (int64_t)r0 * P.ld_rows;
    float* __restrict__ out = P.grad;
    for (uint32_t e = threadIdx.x; e < cnt; e += kEmbThreads) {
      const uint32_t row = e / F, c = e - row * F;
      const int32_t d = dst_rows[row];
      if (d >= 0) out[(int64_t)d * P.ld_grad + c] = in[(int64_t)row * P.ld_rows + c];
    }
  }
}
}  // namespace tfgnn

extern "C" int64_t tfgnn_embedding_launch_count(void) {
  return tfgnn::g_embedding_launches.load(std::memory_order_relaxed);
}

extern "C" int tfgnn_embedding_scatter_rows(const float* rows, int64_t ld_rows, const int32_t* ids, int64_t n, int64_t D,
                                            float* table_grad, int64_t ld_grad, int64_t N, int* bad_flag, void* stream) {
  using namespace tfgnn;
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TFGNN_REQUIRE(n >= 0 && N >= 0 && ld_rows >= 0 && ld_grad >= 0, "tfgnn_embedding_scatter_rows: negative size");
  TFGNN_REQUIRE(D >= 1 && D < kLimit, "tfgnn_embedding_scatter_rows: D must be in [1, 2^31)");
  TFGNN_REQUIRE(ld_rows >= D && ld_grad >= D, "tfgnn_embedding_scatter_rows: a row pitch below D");
  TFGNN_REQUIRE(N < kLimit, "tfgnn_embedding_scatter_rows: 2^31 or more table rows (int32 ids)");
  TFGNN_REQUIRE(n <= N, "tfgnn_embedding_scatter_rows: more rows than the table has (the ids are distinct)");
  TFGNN_REQUIRE(N == 0 || table_grad, "tfgnn_embedding_scatter_rows: NULL table_grad");
  TFGNN_REQUIRE(n == 0 || (rows && ids), "tfgnn_embedding_scatter_rows: NULL rows or ids");
  if (N == 0) return TFGNN_OK;

  EmbParams P;
  memset(&P, 0, sizeof(P));
  P.rows = rows;
  P.ids = ids;
  P.grad = table_grad;
  P.ld_rows = ld_rows;
  P.ld_grad = ld_grad;
  P.n = (int32_t)n;
  P.N = (int32_t)N;
  P.D = (int32_t)D;
  P.rows_per_tile = (int)std::max<int64_t>(1, std::min<int64_t>(kEmbThreads, kEmbTileElems / D));
  P.vec4 = D % 4 == 0 && ld_grad % 4 == 0 && (uintptr_t)table_grad % 16 == 0 &&
           (n == 0 || (ld_rows % 4 == 0 && (uintptr_t)rows % 16 == 0));
  P.bad = bad_flag;
  const int64_t fill_blocks = ceil_div(N, P.rows_per_tile), scatter_blocks = ceil_div(n, P.rows_per_tile);
  TFGNN_REQUIRE(fill_blocks < kLimit, "tfgnn_embedding_scatter_rows: table too large for one grid");
  hipLaunchKernelGGL(embedding_fill_kernel, dim3((unsigned)fill_blocks), dim3(kEmbThreads), 0, (hipStream_t)stream, P);
  TFGNN_LAUNCH_CHECK();
  g_embedding_launches.fetch_add(1, std::memory_order_relaxed);
  if (scatter_blocks == 0) return TFGNN_OK;
  hipLaunchKernelGGL(embedding_scatter_kernel, dim3((unsigned)scatter_blocks), dim3(kEmbThreads), 0, (hipStream_t)stream, P);
  TFGNN_LAUNCH_CHECK();
  g_embedding_launches.fetch_add(1, std::memory_order_relaxed);
  return TFGNN_OK;
}
