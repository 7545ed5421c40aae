// Repair of a tripped split-operand TN product, in stream order and without the host (tn_repair.hpp; include/tfgnn.h
// tfgnn_sp_guard_repair).
//
// The product's loss beyond its guard comes from ONE place: the fp16 per-k factor inv_a[k, blk] inv_b[k] / ref, which holds a
// row 2^-j below its K range's largest with 35 - j bits and drops it at j > 24.  The SP16 operands themselves hold >= 22
// significand bits per element under EXACT power-of-two scales, so the slab of a K range can be recomputed from them in fp32:
//   partial[z][m][n] = sum_{k in range z} (h_a + l_a)[k, m] inv_a[k, blk(m)] * (h_b + l_b)[k, n] inv_b[k]
// with fp32 FMA in ascending k - a fixed order, so a repaired product is reproducible (eager == replay).  (k, block) pairs whose
// scale carries the all-zero marker are skipped exactly as the product kernels skip them (sp_row_holds).  The reference scales
// the reduce pass multiplies back become 1; sp_tn_reduce_kernel then lands the result like any other product's.
//
// A rare path: plain VALU work, a 64 x 64 output tile per 256-thread workgroup (4 x 4 per thread), 16 rows of K staged through
// LDS per step.  One workgroup per (output tile, K range) - the product's own decomposition, so the slabs line up.
//
// The grouped product (K ranges from its split table) is repaired range by range: workgroup (tile, z) looks at trip word z alone,
// rewrites slab z alone and sets the references of range z alone.  What a range's slab holds then depends only on the operands
// and the table, never on which other ranges tripped; the grouped reduce pass adds the slabs in range order as always.
#include "tn_repair.hpp"

#include "sp16.hpp"

namespace tfgnn {

constexpr int RP_TILE = 64, RP_KSTEP = 16;

__global__ void __launch_bounds__(256) sp_tn_repair_kernel(TnRepairArgs a) {
  // the product kernels (earlier on the stream) stored 1 here if a row was beyond their range; 0 (zeroed in front of them): nothing to do
  // (grouped: the word of this workgroup's own K range)
  const int z = blockIdx.y;
  if (*reinterpret_cast<const volatile int*>(a.split_table ? a.trip + z : a.trip) == 0) return;
  typedef _Float16 half4 __attribute__((ext_vector_type(4)));
  __shared__ float4 As[RP_KSTEP][RP_TILE / 4];
  __shared__ float4 Bs[RP_KSTEP][RP_TILE / 4];
  const int t = threadIdx.x;
  const int n_tiles = (int)(a.N / RP_TILE);
  const int tm = blockIdx.x / n_tiles, tn = blockIdx.x - tm * n_tiles;
  int64_t k0 = (int64_t)z * a.k_chunk;
  int64_t k1 = k0 + a.k_chunk < a.K ? k0 + a.k_chunk : a.K;
  if (a.split_table) {
    k0 = a.split_table[2 * z];
    k1 = k0 + a.split_table[2 * z + 1];
  }
  // loads: thread -> (row of the step, 4 columns); products: thread -> 4 x 4 outputs
  const int lr = t >> 4, lc = (t & 15) * 4;
  const int64_t am = (int64_t)tm * RP_TILE + lc;  // first of this thread's 4 columns of A (M % 4 == 0: all four inside or none)
  const int64_t bn = (int64_t)tn * RP_TILE + lc;  // ... of B (N % 64 == 0: always inside)
  const bool a_in = am < a.M;
  const int64_t a_off = (am >> 4) * 64 + (am & 15) * 2, b_off = (bn >> 4) * 64 + (bn & 15) * 2;
  int blk[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) blk[e] = a_in ? (int)((a.a_col0 + am + e) / a.a_sb) : 0;
  const int ty = t >> 4, tx = t & 15;
  float acc[4][4] = {};
  for (int64_t kb = k0; kb < k1; kb += RP_KSTEP) {
    const int64_t k = kb + lr;
    float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
    if (k < k1) {
      const float ib = a.inv_b ? a.inv_b[k] : 1.f;
      const uint8_t* pb = a.B + k * a.ldb + b_off;
      const half4 hb = *reinterpret_cast<const half4*>(pb), lb = *reinterpret_cast<const half4*>(pb + 32);
      vb = make_float4(((float)hb[0] + (float)lb[0]) * ib, ((float)hb[1] + (float)lb[1]) * ib, ((float)hb[2] + (float)lb[2]) * ib,
                       ((float)hb[3] + (float)lb[3]) * ib);
      if (a_in) {
        const uint8_t* pa = a.A + k * a.lda + a_off;
        const half4 ha = *reinterpret_cast<const half4*>(pa), la = *reinterpret_cast<const half4*>(pa + 32);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float ia = a.inv_a[k * a.a_nblk + blk[e]];
          v[e] = sp_row_holds(ia, ib) ? ((float)ha[e] + (float)la[e]) * ia : 0.f;
        }
        va = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    __syncthreads();  // the previous step's products are done with the tiles
    As[lr][lc >> 2] = va;
    Bs[lr][lc >> 2] = vb;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < RP_KSTEP; ++kk) {
      const float4 x = As[kk][ty], y = Bs[kk][tx];
      const float xa[4] = {x.x, x.y, x.z, x.w}, ya[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(xa[i], ya[j], acc[i][j]);
    }
  }
  float* slab = a.partial + (int64_t)z * a.slab;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = (int64_t)tm * RP_TILE + ty * 4 + i;
    if (m < a.M)
      *reinterpret_cast<float4*>(slab + m * a.N + (int64_t)tn * RP_TILE + tx * 4) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
  }
  if (blockIdx.x == 0) {
    // the slabs now hold the sums themselves: the reduce pass multiplies by 1
    if (a.ref_per_split) {
      for (int b = t; b < a.a_nblk; b += 256) a.ref[(int64_t)z * a.a_nblk + b] = 1.f;
    } else if (z == 0) {
      for (int b = t; b < a.a_nblk; b += 256) a.ref[b] = 1.f;
    }
    if (a.split_table) {
      // a grouped launch counts once, however many of its ranges tripped: the first range to flip the tail's last word does it
      if (t == 0 && __hip_atomic_exchange(a.trip + kTnRepairGroupedMaxRanges, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
        __hip_atomic_fetch_add(a.repaired, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (z == 0 && t == 0) {
      __hip_atomic_fetch_add(a.repaired, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// zeroes the grouped product's tail in front of the product (tn_repair_begin)
__global__ void __launch_bounds__(256) sp_tn_repair_clear_kernel(int* __restrict__ words, int n) {
  for (int i = threadIdx.x; i < n; i += 256) words[i] = 0;
}

// ---- state: the switch, the host counter of armed products, one device counter of repaired products per device ----
constexpr int kRepairMaxDevices = 64;
static int g_repair_on = -1;  // -1: not decided yet (environment)
static int64_t g_repair_armed_products = 0;
static unsigned long long* g_repair_counter[kRepairMaxDevices] = {};

bool tn_repair_armed() {
  if (g_repair_on < 0) {
    const char* e = getenv("TFGNN_GUARD_REPAIR");
    g_repair_on = (e && atoi(e) != 0) ? 1 : 0;
  }
  return g_repair_on == 1;
}

// the current device's counter; allocated (zero) at first use - never inside a stream capture (callers check)
static unsigned long long* repair_counter(bool allocate) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kRepairMaxDevices) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (!g_repair_counter[dev] && allocate) {
    unsigned long long* p = nullptr;
    if (hipMalloc((void**)&p, 256) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    if (hipMemset(p, 0, 256) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(p);
      return nullptr;
    }
    g_repair_counter[dev] = p;
  }
  return g_repair_counter[dev];
}

static bool repair_stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {
    (void)hipGetLastError();
    return true;  // (the legacy stream while another stream captures: an implicit-capture error)
  }
  return st != hipStreamCaptureStatusNone;
}

int tn_repair_begin(int* trip_word, size_t tail_bytes, hipStream_t s) {
  if (!repair_counter(false)) {  // armed through the environment (or on another device): the counter does not exist yet
    TFGNN_REQUIRE(!repair_stream_capturing(s),
                  "tfgnn_sp_gemm_tn: repair is armed but its device counter does not exist yet and the stream is capturing "
                  "(call tfgnn_sp_guard_repair(1) or run one product before the capture)");
    TFGNN_REQUIRE(repair_counter(true), "tfgnn_sp_gemm_tn: no device memory for the repair counter");
  }
  if (tail_bytes <= sizeof(int)) {
    TFGNN_HIP_CHECK(hipMemsetAsync(trip_word, 0, tail_bytes, s));
  } else {
    // the grouped product's tail (trip words + the counted word).  Not a memset node: measured on the MI355X, a product captured
    // into a hipGraph behind a 2304-byte memset node lost its trip words in every replay but the first (the 4-byte node of the
    // plain products never did; eager calls were right with either) - a kernel node orders like the kernels around it
    const int words = (int)(tail_bytes / sizeof(int));
    hipLaunchKernelGGL(sp_tn_repair_clear_kernel, dim3(1), dim3(256), 0, s, trip_word, words);
    TFGNN_LAUNCH_CHECK();
  }
  ++g_repair_armed_products;
  return TFGNN_OK;
}

int tn_repair_enqueue(TnRepairArgs a, hipStream_t s) {
  a.repaired = repair_counter(false);
  TFGNN_REQUIRE(a.repaired && a.trip && a.N % RP_TILE == 0 && a.M % 4 == 0 && a.splits >= 1 &&
                    a.splits <= (a.split_table ? kTnRepairGroupedMaxRanges : 65535) && (!a.split_table || a.ref_per_split),
                "tfgnn_sp_gemm_tn: repair pass cannot run (no counter, or a shape the product itself rejects)");
  const int64_t tiles = ceil_div(a.M, RP_TILE) * (a.N / RP_TILE);
  hipLaunchKernelGGL(sp_tn_repair_kernel, dim3((unsigned)tiles, (unsigned)a.splits), dim3(256), 0, s, a);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}

}  // namespace tfgnn

using namespace tfgnn;

extern "C" int tfgnn_sp_guard_repair(int on) {
  const int prev = tn_repair_armed() ? 1 : 0;
  if (on < 0) return prev;
  if (on) {
    if (!repair_counter(false)) {
      TFGNN_REQUIRE(!repair_stream_capturing(nullptr), "tfgnn_sp_guard_repair: arming allocates; not legal while a stream is capturing");
      if (!repair_counter(true)) {
        set_error("tfgnn_sp_guard_repair: no device memory for the repair counter");
        return TFGNN_ERR_HIP;
      }
    }
    g_repair_on = 1;
  } else {
    g_repair_on = 0;
  }
  return prev;
}

extern "C" int tfgnn_sp_repair_stats(int64_t* out2, int reset) {
  TFGNN_REQUIRE(out2, "tfgnn_sp_repair_stats: null pointer");
  TFGNN_REQUIRE(!repair_stream_capturing(nullptr), "tfgnn_sp_repair_stats: waits for the device; not legal while a stream is capturing");
  TFGNN_HIP_CHECK(hipDeviceSynchronize());
  unsigned long long v = 0;
  unsigned long long* c = repair_counter(false);
  if (c) TFGNN_HIP_CHECK(hipMemcpy(&v, c, sizeof(v), hipMemcpyDeviceToHost));
  out2[0] = g_repair_armed_products;
  out2[1] = (int64_t)v;
  if (reset) {
    g_repair_armed_products = 0;
    if (c) TFGNN_HIP_CHECK(hipMemset(c, 0, sizeof(v)));
  }
  return TFGNN_OK;
}
