// Optimizer step: clipping + SGD / RMSprop / Adam over many (variable, gradient) pairs per call, learning rate and step
// counter on the device (include/tfgnn.h "Optimizer step"; models/graph_task_model.py:224-324).
#include <atomic>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace tfgnn {

constexpr int OPT_CHUNK = 32;          // tensors per launch (the table travels as the kernel argument)
constexpr int OPT_THREADS = 256;
constexpr int OPT_UPD_ELEMS = 2048;    // elements per workgroup of the update: two float4 per thread, loaded together
constexpr int OPT_SUM_ELEMS = 8192;    // elements per workgroup of the squared-sum pass: 8 float4 per thread, loaded together
constexpr int OPT_ROW_CHUNK = TFGNN_OPT_MAX_ROW_TENSORS;  // row tensors of a call: one update launch for all of them
constexpr int OPT_ROW_TILE_ELEMS = 8192;  // floats of a row tensor's tile (whole rows; one row when a row is longer)

enum { OPT_K_SGD = 0, OPT_K_SGD_MOM = 1, OPT_K_RMS = 2, OPT_K_RMS_MOM = 3, OPT_K_ADAM = 4 };

struct OptEntry {  // one tensor of a launch (64 bytes); a contiguous tensor is one row of n elements
  float* w;
  const float* g;
  float* s0;
  float* s1;
  uint32_t ldw, ldg, cols, n;
  uint32_t blk0;    // first workgroup of this tensor in its update launch
  uint32_t part0;   // first partial sum of this tensor in the workspace (= its first workgroup of the squared-sum pass)
  uint32_t nparts;
  uint32_t vec;     // 16-byte accesses: every row a whole number of aligned float4 (contiguous: + a scalar tail)
};

struct OptParams {
  int kind, clip;
  float clip_value, momentum, rho, beta_1, beta_2, epsilon;
  int schedule;
  float lr, lr_initial, lr_final, power, warmup, decay;
  int n;                      // tensors in this launch
  unsigned long long* state;  // [0] iterations, [1] ticket
  double* partials;
  uint32_t part_base;         // partial index of this launch's first squared-sum workgroup
  uint32_t total_parts;       // partial sums of the whole call
  uint32_t blocks;            // workgroups of this launch
  int advance;                // the last update launch of the call: its last workgroup advances the counter
};

struct OptTable {
  OptParams p;
  OptEntry e[OPT_CHUNK];
};

// the squared-sum launch that also takes the row tensors of a call (as the [n, cols] tensors their gradients are)
struct OptSumRowsTable {
  OptParams p;
  OptEntry e[OPT_CHUNK + OPT_ROW_CHUNK];
};

struct OptRowEntry {  // one row tensor of the row-update launch
  float* w;           // the table [N, cols], pitch ldw
  const float* g;     // [n, cols], pitch ldg
  const int32_t* ids;
  float* s0;          // [N * cols]
  float* s1;
  int* bad;
  int64_t ldw, ldg;
  uint32_t n, N, cols;
  uint32_t rows_per_tile;
  uint32_t blk0;      // first workgroup of this tensor in the launch
  uint32_t part0;     // its partial sums in the workspace
  uint32_t nparts;
  uint32_t vec;       // 16-byte accesses: cols % 4 == 0, both pitches multiples of 4, every base aligned
  uint32_t quad_elems;  // !vec: the elements of the [n, cols] gradient the dense step would compute four at a time
};

struct OptRowTable {
  OptParams p;  // p.n: row tensors of the launch (0: nothing to update, the launch only advances the counter)
  OptRowEntry r[OPT_ROW_CHUNK];
};

typedef const __attribute__((address_space(4))) OptTable* opt_table_cptr;
typedef const __attribute__((address_space(4))) OptParams* opt_params_cptr;
typedef const __attribute__((address_space(4))) OptEntry* opt_entry_cptr;
typedef const __attribute__((address_space(4))) OptRowTable* opt_row_table_cptr;
typedef const __attribute__((address_space(4))) OptRowEntry* opt_row_entry_cptr;

// The table is the kernel's only explicit argument, at offset 0 of the argument segment: fields are read from there with
// scalar loads (indexing the by-value parameter with a run-time entry index would copy it to scratch first - aux_jobs.hip).
__device__ __forceinline__ opt_table_cptr opt_table() { return (opt_table_cptr)__builtin_amdgcn_kernarg_segment_ptr(); }

__device__ __forceinline__ uint64_t opt_row_off(uint32_t e, uint32_t cols, uint32_t ld, uint32_t n) {
  if (cols == n) return e;  // one row (contiguous)
  const uint32_t r = e / cols;
  return (uint64_t)r * ld + (e - r * cols);
}

// sum over the threads of a workgroup, in a fixed order (every workgroup that sums the same values gets the same bits)
__device__ __forceinline__ double opt_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read by a previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- launch 1 of the norm modes: per-workgroup partial sums of g^2 -> partials[part_base + blockIdx.x] ----
// (both tables begin with the parameters followed by the entries: the body takes the two addresses)
__device__ __forceinline__ void opt_sumsq_body(opt_params_cptr P, opt_entry_cptr entries, double* red) {
  const uint32_t b = P->part_base + blockIdx.x;
  int k = 0;
  const int n_t = P->n;
  while (k + 1 < n_t && b >= entries[k + 1].part0) ++k;
  const opt_entry_cptr E = &entries[k];
  const float* __restrict__ g = E->g;
  const uint32_t n = E->n, cols = E->cols, ldg = E->ldg;
  const uint32_t lb = b - E->part0;
  double acc = 0.0;
  if (E->vec) {
    constexpr int Q = OPT_SUM_ELEMS / 4 / OPT_THREADS;
    const uint32_t nq = n >> 2;
    const uint32_t q0 = lb * (OPT_SUM_ELEMS / 4);
    float4 v[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {  // every load first, then the sums
      const uint32_t q = q0 + i * OPT_THREADS + threadIdx.x;
      v[i] = q < nq ? *reinterpret_cast<const float4*>(g + opt_row_off(q * 4, cols, ldg, n)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      acc = fma((double)v[i].x, (double)v[i].x, acc);
      acc = fma((double)v[i].y, (double)v[i].y, acc);
      acc = fma((double)v[i].z, (double)v[i].z, acc);
      acc = fma((double)v[i].w, (double)v[i].w, acc);
    }
    if (lb == 0 && nq * 4 + threadIdx.x < n) {  // contiguous tail of n % 4 elements
      const float x = g[nq * 4 + threadIdx.x];
      acc = fma((double)x, (double)x, acc);
    }
  } else {
    const uint32_t e0 = lb * OPT_SUM_ELEMS, e1 = min(e0 + OPT_SUM_ELEMS, n);
#pragma unroll 8
    for (uint32_t e = e0 + threadIdx.x; e < e1; e += OPT_THREADS) {
      const float x = g[opt_row_off(e, cols, ldg, n)];
      acc = fma((double)x, (double)x, acc);
    }
  }
  const double s = opt_block_sum(acc, red);
  if (threadIdx.x == 0) P->partials[b] = s;
}

__global__ void __launch_bounds__(OPT_THREADS) opt_sumsq_kernel(OptTable table) {
  (void)table;
  __shared__ double red[OPT_THREADS / 64];
  const opt_table_cptr T = opt_table();
  opt_sumsq_body(&T->p, T->e, red);
}

__global__ void __launch_bounds__(OPT_THREADS) opt_sumsq_rows_kernel(OptSumRowsTable table) {
  (void)table;
  __shared__ double red[OPT_THREADS / 64];
  const auto T = (const __attribute__((address_space(4))) OptSumRowsTable*)__builtin_amdgcn_kernarg_segment_ptr();
  opt_sumsq_body(&T->p, T->e, red);
}

struct OptCoef {
  float lr;  // Adam: alpha
  float mu, rho, one_minus_rho, eps, one_minus_b1, one_minus_b2;
  int clip;
  float c;     // clip value / norm
  float den;   // TFGNN_CLIP_NORM: max(|g|, c)
  float scale; // TFGNN_CLIP_GLOBAL_NORM
};

__device__ __forceinline__ float opt_clip(float g, const OptCoef& k) {
  switch (k.clip) {
    case TFGNN_CLIP_VALUE:
      return fmaxf(fminf(g, k.c), -k.c);  // clip_by_value: minimum, then maximum
    case TFGNN_CLIP_NORM:
      return g * k.c / k.den;             // clip_by_norm: t * clip_norm / maximum(l2norm, clip_norm)
    case TFGNN_CLIP_GLOBAL_NORM:
      return g * k.scale;
    default:
      return g;
  }
}

template <int KIND>
__device__ __forceinline__ void opt_elem(float& w, float g, float& s0, float& s1, const OptCoef& k) {
  g = opt_clip(g, k);
  if (KIND == OPT_K_SGD) {
    w -= k.lr * g;
  } else if (KIND == OPT_K_SGD_MOM) {
    s0 = s0 * k.mu - k.lr * g;
    w += s0;
  } else if (KIND == OPT_K_RMS) {
    s0 = k.rho * s0 + k.one_minus_rho * (g * g);
    w -= k.lr * g / (sqrtf(s0) + k.eps);
  } else if (KIND == OPT_K_RMS_MOM) {
    s0 += (g * g - s0) * k.one_minus_rho;
    s1 = s1 * k.mu + k.lr * g * rsqrtf(s0 + k.eps);
    w -= s1;
  } else {  // Adam
    s0 += (g - s0) * k.one_minus_b1;
    s1 += (g * g - s1) * k.one_minus_b2;
    w -= s0 * k.lr / (sqrtf(s1) + k.eps);
  }
}

constexpr bool opt_has_s0(int kind) { return kind != OPT_K_SGD; }
constexpr bool opt_has_s1(int kind) { return kind == OPT_K_RMS_MOM || kind == OPT_K_ADAM; }

// the learning rate at step = (float)iterations (polynomial_warmup_and_decay_schedule.py:90-111, fp32 like the float32 step Keras
// passes in)
__device__ __forceinline__ float opt_learning_rate(opt_params_cptr P, float step) {
  const float lr = P->lr;
  if (!P->schedule) return lr;
  const float warmup = P->warmup, decay = P->decay, power = P->power;
  if (step <= warmup) return (lr - P->lr_initial) * powf(step / warmup, power) + P->lr_initial;
  const float s = fminf(step - warmup, decay);
  return (lr - P->lr_final) * powf(1.f - s / decay, power) + P->lr_final;
}

// sum of partials[lo, hi) in a fixed order: every workgroup of a tensor (or of the call) computes the same bits
__device__ __forceinline__ double opt_sum_partials(const double* __restrict__ p, uint32_t lo, uint32_t hi, double* red) {
  double acc = 0.0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += OPT_THREADS) acc += p[i];
  return opt_block_sum(acc, red);
}

// the coefficients of a workgroup's tensor at the counter value `it`: the learning rate of the schedule (Adam: alpha at
// t = it + 1) and the clip factors from the partial sums [part0, part0 + nparts) of the tensor / of the whole call
template <int KIND>
__device__ __forceinline__ OptCoef opt_coefficients(opt_params_cptr P, unsigned long long it, uint32_t part0, uint32_t nparts,
                                                    double* red) {
  OptCoef c;
  c.lr = opt_learning_rate(P, (float)it);
  c.mu = P->momentum;
  c.rho = P->rho;
  c.one_minus_rho = 1.f - P->rho;
  c.eps = P->epsilon;
  c.one_minus_b1 = 1.f - P->beta_1;
  c.one_minus_b2 = 1.f - P->beta_2;
  if (KIND == OPT_K_ADAM) {
    const float t = (float)(it + 1);
    const float b1p = powf(P->beta_1, t), b2p = powf(P->beta_2, t);
    c.lr = c.lr * (sqrtf(1.f - b2p) / (1.f - b1p));
  }
  c.clip = P->clip;
  c.c = P->clip_value;
  c.den = 1.f;
  c.scale = 1.f;
  if (c.clip == TFGNN_CLIP_NORM) {
    const float norm = (float)sqrt(opt_sum_partials(P->partials, part0, part0 + nparts, red));
    c.den = fmaxf(norm, c.c);
  } else if (c.clip == TFGNN_CLIP_GLOBAL_NORM) {
    const float norm = (float)sqrt(opt_sum_partials(P->partials, 0, P->total_parts, red));
    // clip_by_global_norm: clip_norm * minimum(1 / use_norm, 1 / clip_norm), NaN when the norm is not finite
    c.scale = isfinite(norm) ? c.c * fminf(1.f / norm, 1.f / c.c) : __builtin_nanf("");
  }
  return c;
}

// the ticket of a call's last update launch: the workgroup that arrives last has seen every other one read the counter and
// advances it; it resets the ticket for the next call.  Relaxed: what orders a workgroup's read of the counter before its add is
// that thread 0 has consumed the value (LDS store + barrier in the caller); the update's own stores need no ordering (the next
// reader is another launch), and a release here would write the L2 back once per workgroup (buffer_wbl2; measured: it doubled
// the call's time).
__device__ __forceinline__ void opt_advance(opt_params_cptr P, unsigned long long it) {
  if (P->advance && threadIdx.x == 0) {
    unsigned long long* st = P->state;
    const unsigned long long t = __hip_atomic_fetch_add(st + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == (unsigned long long)P->blocks - 1) {
      __hip_atomic_store(st + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(st, it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- the update: one launch per chunk ----
template <int KIND>
__global__ void __launch_bounds__(OPT_THREADS) opt_update_kernel(OptTable table) {
  (void)table;
  __shared__ double red[OPT_THREADS / 64];
  const opt_table_cptr T = opt_table();
  const uint32_t b = blockIdx.x;
  int k = 0;
  const int n_t = T->p.n;
  while (k + 1 < n_t && b >= T->e[k + 1].blk0) ++k;
  const opt_entry_cptr E = &T->e[k];

  // every workgroup reads the counter (thread 0, the thread that later takes the ticket: its release add is ordered after this
  // load) before it arrives at the ticket below: none sees this call's advance
  __shared__ unsigned long long it_shared;
  if (threadIdx.x == 0) it_shared = __hip_atomic_load(T->p.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const unsigned long long it = it_shared;
  const OptCoef c = opt_coefficients<KIND>(&T->p, it, E->part0, E->nparts, red);

  float* __restrict__ w = E->w;
  const float* __restrict__ g = E->g;
  float* __restrict__ s0 = E->s0;
  float* __restrict__ s1 = E->s1;
  const uint32_t n = E->n, cols = E->cols, ldw = E->ldw, ldg = E->ldg;
  const uint32_t lb = b - E->blk0;
  if (E->vec) {
    const uint32_t nq = n >> 2;
    const uint32_t q0 = lb * (OPT_UPD_ELEMS / 4);
    constexpr int U = OPT_UPD_ELEMS / 4 / OPT_THREADS;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 wv[U], gv[U], a[U], v[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {  // every load first
      const uint32_t q = q0 + i * OPT_THREADS + threadIdx.x;
      wv[i] = gv[i] = a[i] = v[i] = zero;
      if (q < nq) {
        wv[i] = *reinterpret_cast<const float4*>(w + opt_row_off(q * 4, cols, ldw, n));
        gv[i] = *reinterpret_cast<const float4*>(g + opt_row_off(q * 4, cols, ldg, n));
        if (opt_has_s0(KIND)) a[i] = *reinterpret_cast<const float4*>(s0 + q * 4);
        if (opt_has_s1(KIND)) v[i] = *reinterpret_cast<const float4*>(s1 + q * 4);
      }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const uint32_t q = q0 + i * OPT_THREADS + threadIdx.x;
      if (q < nq) {
        opt_elem<KIND>(wv[i].x, gv[i].x, a[i].x, v[i].x, c);
        opt_elem<KIND>(wv[i].y, gv[i].y, a[i].y, v[i].y, c);
        opt_elem<KIND>(wv[i].z, gv[i].z, a[i].z, v[i].z, c);
        opt_elem<KIND>(wv[i].w, gv[i].w, a[i].w, v[i].w, c);
        *reinterpret_cast<float4*>(w + opt_row_off(q * 4, cols, ldw, n)) = wv[i];
        if (opt_has_s0(KIND)) *reinterpret_cast<float4*>(s0 + q * 4) = a[i];
        if (opt_has_s1(KIND)) *reinterpret_cast<float4*>(s1 + q * 4) = v[i];
      }
    }
    if (lb == 0 && nq * 4 + threadIdx.x < n) {  // contiguous tail
      const uint32_t e = nq * 4 + threadIdx.x;
      float a = opt_has_s0(KIND) ? s0[e] : 0.f, v = opt_has_s1(KIND) ? s1[e] : 0.f;
      opt_elem<KIND>(w[e], g[e], a, v, c);
      if (opt_has_s0(KIND)) s0[e] = a;
      if (opt_has_s1(KIND)) s1[e] = v;
    }
  } else {
    const uint32_t e0 = lb * OPT_UPD_ELEMS;
#pragma unroll 4
    for (int i = 0; i < OPT_UPD_ELEMS / OPT_THREADS; ++i) {
      const uint32_t e = e0 + i * OPT_THREADS + threadIdx.x;
      if (e < n) {
        float a = opt_has_s0(KIND) ? s0[e] : 0.f, v = opt_has_s1(KIND) ? s1[e] : 0.f;
        float& wr = w[opt_row_off(e, cols, ldw, n)];
        float wv = wr;
        opt_elem<KIND>(wv, g[opt_row_off(e, cols, ldg, n)], a, v, c);
        wr = wv;
        if (opt_has_s0(KIND)) s0[e] = a;
        if (opt_has_s1(KIND)) s1[e] = v;
      }
    }
  }

  opt_advance(&T->p, it);
}

// ---- the row update: one launch for every row tensor of a call (include/tfgnn.h "The row-sparse step") ----
// A workgroup takes rows_per_tile rows of grad_rows.  One thread per row reads the row's id, checks it against N and leaves it
// in LDS (-1: skipped, *bad set); then the whole workgroup walks the tile's floats, consecutive lanes on consecutive float4 of
// a row (without float4 accesses: on consecutive quads of the gradient's flat index space, see there): w, g and the slots are
// loaded, then opt_elem runs, then w and the slots are stored.  The ids are distinct and every element has one owner, so no
// two threads of the launch touch the same element: plain stores.  Table and slot offsets are 64-bit (N * cols may pass 2^31);
// every access is to a row < N (value, slots) or < n (grad_rows, ids) and a column < cols.
template <int KIND>
__global__ void __launch_bounds__(OPT_THREADS) opt_update_rows_kernel(OptRowTable table) {
  (void)table;
  __shared__ double red[OPT_THREADS / 64];
  __shared__ int32_t dst_rows[OPT_THREADS + 3];
  __shared__ unsigned long long it_shared;
  const opt_row_table_cptr T = (opt_row_table_cptr)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t b = blockIdx.x;
  const int n_t = T->p.n;
  int k = 0;
  while (k + 1 < n_t && b >= T->r[k + 1].blk0) ++k;
  const opt_row_entry_cptr E = &T->r[k];

  // the counter is read by the thread that later takes the ticket, as in opt_update_kernel
  if (threadIdx.x == 0) it_shared = __hip_atomic_load(T->p.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t rows_per_tile = n_t > 0 ? E->rows_per_tile : 0u;
  const uint32_t r0 = (b - (n_t > 0 ? E->blk0 : 0u)) * rows_per_tile;  // < n < 2^31
  const uint32_t rows = n_t > 0 ? min(rows_per_tile, E->n - r0) : 0u;
  // the tile's ids and, for a quad that starts in the tile and ends in the next rows, up to three more (rows_per_tile <= OPT_THREADS)
  const uint32_t ids_in_lds = rows > 0 ? min(rows + 3u, E->n - r0) : 0u;
  for (uint32_t i = threadIdx.x; i < ids_in_lds; i += OPT_THREADS) {
    int32_t id = E->ids[r0 + i];
    if ((uint32_t)id >= E->N) {
      id = -1;
      if (E->bad) *E->bad = 1;
    }
    dst_rows[i] = id;
  }
  __syncthreads();
  const unsigned long long it = it_shared;
  if (rows > 0) {  // uniform over the workgroup
    const OptCoef c = opt_coefficients<KIND>(&T->p, it, E->part0, E->nparts, red);
    float* __restrict__ w = E->w;
    float* __restrict__ s0 = E->s0;
    float* __restrict__ s1 = E->s1;
    const int64_t ldw = E->ldw, ldg = E->ldg, cols = E->cols;
    const float* __restrict__ g = E->g + (int64_t)r0 * ldg;  // local rows from here on
    if (E->vec) {
      const uint32_t F4 = E->cols >> 2;
      const uint32_t cnt = rows * F4;  // <= the tile, or one row of cols < 2^31 floats
      for (uint32_t e = threadIdx.x; e < cnt; e += OPT_THREADS) {
        const uint32_t row = e / F4, c4 = (e - row * F4) * 4u;
        const int32_t d = dst_rows[row];
        if (d < 0) continue;
        float* wp = w + ((int64_t)d * ldw + c4);
        const int64_t so = (int64_t)d * cols + c4;
        float4 wv = *reinterpret_cast<const float4*>(wp);  // every load first
        const float4 gv = *reinterpret_cast<const float4*>(g + ((int64_t)row * ldg + c4));
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), v = a;
        if (opt_has_s0(KIND)) a = *reinterpret_cast<const float4*>(s0 + so);
        if (opt_has_s1(KIND)) v = *reinterpret_cast<const float4*>(s1 + so);
        opt_elem<KIND>(wv.x, gv.x, a.x, v.x, c);
        opt_elem<KIND>(wv.y, gv.y, a.y, v.y, c);
        opt_elem<KIND>(wv.z, gv.z, a.z, v.z, c);
        opt_elem<KIND>(wv.w, gv.w, a.w, v.w, c);
        *reinterpret_cast<float4*>(wp) = wv;
        if (opt_has_s0(KIND)) *reinterpret_cast<float4*>(s0 + so) = a;
        if (opt_has_s1(KIND)) *reinterpret_cast<float4*>(s1 + so) = v;
      }
    } else {
      // Without float4 accesses.  opt_update_kernel computes the elements of an aligned contiguous tensor four at a time and
      // the last numel % 4 (and every element of a tensor it cannot read as float4) one at a time, and the compiler contracts
      // the two forms of opt_elem differently.  The element arithmetic here is that of the dense step at the element's place in
      // the [n, cols] gradient: quads of four consecutive elements of its flat index space (they may cross rows), then the
      // rest one at a time.  A workgroup owns the quads that START in its tile and the single elements of its tile.
      const uint32_t F = E->cols;
      const uint32_t e_lo = r0 * F, e_hi = e_lo + rows * F;  // the tile's flat range: n * cols < 2^31
      const uint32_t quad_end = min(e_hi, E->quad_elems);     // elements below quad_elems (a multiple of 4) go in quads
      for (uint32_t e0 = ((e_lo + 3u) & ~3u) + 4u * threadIdx.x; e0 < quad_end; e0 += 4u * OPT_THREADS) {
        uint32_t row = e0 / F - r0, col = e0 - (row + r0) * F;  // row: local, below rows + 3 (ids_in_lds)
        float* wp[4];
        int64_t so[4];
        float4 wv, gv, a = make_float4(0.f, 0.f, 0.f, 0.f), v = a;
        float* const wq[4] = {&wv.x, &wv.y, &wv.z, &wv.w};
        float* const gq[4] = {&gv.x, &gv.y, &gv.z, &gv.w};
        float* const aq[4] = {&a.x, &a.y, &a.z, &a.w};
        float* const vq[4] = {&v.x, &v.y, &v.z, &v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // every load first
          const int32_t d = dst_rows[row];
          wp[j] = d >= 0 ? w + ((int64_t)d * ldw + col) : nullptr;
          so[j] = (int64_t)d * cols + col;
          *wq[j] = *gq[j] = 0.f;
          if (d >= 0) {
            *wq[j] = *wp[j];
            *gq[j] = g[(int64_t)row * ldg + col];
            if (opt_has_s0(KIND)) *aq[j] = s0[so[j]];
            if (opt_has_s1(KIND)) *vq[j] = s1[so[j]];
          }
          if (++col == F) {
            col = 0;
            ++row;
          }
        }
        opt_elem<KIND>(wv.x, gv.x, a.x, v.x, c);
        opt_elem<KIND>(wv.y, gv.y, a.y, v.y, c);
        opt_elem<KIND>(wv.z, gv.z, a.z, v.z, c);
        opt_elem<KIND>(wv.w, gv.w, a.w, v.w, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (wp[j]) {
            *wp[j] = *wq[j];
            if (opt_has_s0(KIND)) s0[so[j]] = *aq[j];
            if (opt_has_s1(KIND)) s1[so[j]] = *vq[j];
          }
        }
      }
      for (uint32_t e = max(e_lo, E->quad_elems) + threadIdx.x; e < e_hi; e += OPT_THREADS) {
        const uint32_t row = e / F - r0, col = e - (row + r0) * F;
        const int32_t d = dst_rows[row];
        if (d < 0) continue;
        float* wp = w + ((int64_t)d * ldw + col);
        const int64_t so = (int64_t)d * cols + col;
        float wv = *wp;
        const float gv = g[(int64_t)row * ldg + col];
        float a = opt_has_s0(KIND) ? s0[so] : 0.f, v = opt_has_s1(KIND) ? s1[so] : 0.f;
        opt_elem<KIND>(wv, gv, a, v, c);
        *wp = wv;
        if (opt_has_s0(KIND)) s0[so] = a;
        if (opt_has_s1(KIND)) s1[so] = v;
      }
    }
  }
  opt_advance(&T->p, it);
}

__global__ void opt_iterations_get_kernel(const long long* state, long long* out) { *out = state[0]; }
__global__ void opt_iterations_set_kernel(long long* state, long long value) {
  state[0] = value;
  state[1] = 0;
}

static std::atomic<int64_t> g_opt_launches{0};

static inline bool opt_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the entries of a call (empty tensors dropped): per entry its workgroup counts; -> total partial sums
struct OptPlan {
  std::vector<OptEntry> e;
  std::vector<uint32_t> upd_blocks;
  uint64_t total_parts = 0;
};

static int opt_plan(const tfgnn_opt_tensor* t, int n, int kind, float momentum, OptPlan& plan) {
  TFGNN_REQUIRE(n >= 0 && (n == 0 || t != nullptr), "tfgnn_optimizer: bad tensor list (n = %d)", n);
  const bool need0 = kind != TFGNN_OPT_SGD || momentum > 0.f;
  const bool need1 = kind == TFGNN_OPT_ADAM || (kind == TFGNN_OPT_RMSPROP && momentum > 0.f);
  for (int i = 0; i < n; ++i) {
    const tfgnn_opt_tensor& d = t[i];
    TFGNN_REQUIRE(d.rows >= 0 && d.cols >= 0, "tfgnn_optimizer: tensor %d has a negative shape", i);
    const int64_t numel = d.rows * d.cols;
    if (numel == 0) continue;
    TFGNN_REQUIRE(numel < (1ll << 31), "tfgnn_optimizer: tensor %d has %lld elements (at most 2^31 - 1)", i, (long long)numel);
    TFGNN_REQUIRE(d.value && d.grad, "tfgnn_optimizer: tensor %d: NULL value or gradient", i);
    TFGNN_REQUIRE((!need0 || d.slot0) && (!need1 || d.slot1), "tfgnn_optimizer: tensor %d: NULL slot the optimizer needs", i);
    TFGNN_REQUIRE(d.rows == 1 || (d.ld_value >= d.cols && d.ld_grad >= d.cols),
                  "tfgnn_optimizer: tensor %d: row strides %lld / %lld below the width %lld", i, (long long)d.ld_value,
                  (long long)d.ld_grad, (long long)d.cols);
    TFGNN_REQUIRE(d.ld_value < (1ll << 32) && d.ld_grad < (1ll << 32), "tfgnn_optimizer: tensor %d: row stride too large", i);
    OptEntry e{};
    e.w = d.value;
    e.g = d.grad;
    e.s0 = need0 ? d.slot0 : nullptr;
    e.s1 = need1 ? d.slot1 : nullptr;
    e.n = (uint32_t)numel;
    const bool contiguous = d.rows == 1 || (d.ld_value == d.cols && d.ld_grad == d.cols);
    e.cols = contiguous ? e.n : (uint32_t)d.cols;
    e.ldw = contiguous ? e.n : (uint32_t)d.ld_value;
    e.ldg = contiguous ? e.n : (uint32_t)d.ld_grad;
    const bool aligned = opt_aligned(e.w) && opt_aligned(e.g) && (!e.s0 || opt_aligned(e.s0)) && (!e.s1 || opt_aligned(e.s1));
    e.vec = aligned && (contiguous || (e.cols % 4 == 0 && e.ldw % 4 == 0 && e.ldg % 4 == 0));
    e.nparts = (uint32_t)ceil_div(numel, OPT_SUM_ELEMS);
    e.part0 = (uint32_t)plan.total_parts;
    plan.total_parts += e.nparts;
    plan.e.push_back(e);
    plan.upd_blocks.push_back((uint32_t)ceil_div(numel, OPT_UPD_ELEMS));
  }
  TFGNN_REQUIRE(plan.total_parts < (1ull << 31), "tfgnn_optimizer: too many elements");
  return TFGNN_OK;
}

static size_t opt_workspace_bytes(const OptPlan& plan, int clip) {
  if (clip != TFGNN_CLIP_NORM && clip != TFGNN_CLIP_GLOBAL_NORM) return 0;
  return (size_t)plan.total_parts * sizeof(double);
}

// the row tensors of a call: per tensor its entry of the row-update launch and - as the [n, cols] tensor grad_rows is - its
// entry of the squared-sum pass, after the dense tensors of `plan` (tensors with n == 0 dropped)
struct OptRowPlan {
  std::vector<OptRowEntry> r;
  std::vector<OptEntry> sum;
  uint32_t blocks = 0;
};

static int opt_plan_rows(const tfgnn_opt_row_tensor* t, int n_rows, int kind, float momentum, OptPlan& plan, OptRowPlan& rows) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TFGNN_REQUIRE(n_rows >= 0 && (n_rows == 0 || t != nullptr), "tfgnn_optimizer: bad row tensor list (n_rows = %d)", n_rows);
  TFGNN_REQUIRE(n_rows <= OPT_ROW_CHUNK, "tfgnn_optimizer: %d row tensors (at most %d to a call)", n_rows, OPT_ROW_CHUNK);
  const bool need0 = kind != TFGNN_OPT_SGD || momentum > 0.f;
  const bool need1 = kind == TFGNN_OPT_ADAM || (kind == TFGNN_OPT_RMSPROP && momentum > 0.f);
  uint64_t blocks = 0;
  for (int i = 0; i < n_rows; ++i) {
    const tfgnn_opt_row_tensor& d = t[i];
    TFGNN_REQUIRE(d.n >= 0 && d.N >= 0, "tfgnn_optimizer: row tensor %d has a negative size", i);
    TFGNN_REQUIRE(d.cols >= 1 && d.cols < kLimit, "tfgnn_optimizer: row tensor %d: cols must be in [1, 2^31)", i);
    TFGNN_REQUIRE(d.N < kLimit, "tfgnn_optimizer: row tensor %d: 2^31 or more table rows (int32 ids)", i);
    TFGNN_REQUIRE(d.n <= d.N, "tfgnn_optimizer: row tensor %d: more rows than the table has (the ids are distinct)", i);
    TFGNN_REQUIRE(d.ld_value >= d.cols && d.ld_grad >= d.cols,
                  "tfgnn_optimizer: row tensor %d: row pitches %lld / %lld below the width %lld", i, (long long)d.ld_value,
                  (long long)d.ld_grad, (long long)d.cols);
    TFGNN_REQUIRE(d.ld_grad < (1ll << 32), "tfgnn_optimizer: row tensor %d: gradient row pitch too large", i);
    const int64_t numel = d.n * d.cols;  // < 2^62
    TFGNN_REQUIRE(numel < kLimit, "tfgnn_optimizer: row tensor %d: its gradient has %lld elements (at most 2^31 - 1)", i,
                  (long long)numel);
    if (d.n == 0) continue;
    TFGNN_REQUIRE(d.value && d.grad_rows && d.ids, "tfgnn_optimizer: row tensor %d: NULL value, gradient rows or ids", i);
    TFGNN_REQUIRE((!need0 || d.slot0) && (!need1 || d.slot1), "tfgnn_optimizer: row tensor %d: NULL slot the optimizer needs", i);
    OptRowEntry e{};
    e.w = d.value;
    e.g = d.grad_rows;
    e.ids = d.ids;
    e.s0 = need0 ? d.slot0 : nullptr;
    e.s1 = need1 ? d.slot1 : nullptr;
    e.bad = d.bad_flag;
    e.ldw = d.ld_value;
    e.ldg = d.ld_grad;
    e.n = (uint32_t)d.n;
    e.N = (uint32_t)d.N;
    e.cols = (uint32_t)d.cols;
    e.rows_per_tile = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(OPT_THREADS, OPT_ROW_TILE_ELEMS / d.cols));
    e.vec = d.cols % 4 == 0 && d.ld_value % 4 == 0 && d.ld_grad % 4 == 0 && opt_aligned(e.w) && opt_aligned(e.g) &&
            (!e.s0 || opt_aligned(e.s0)) && (!e.s1 || opt_aligned(e.s1));
    e.blk0 = (uint32_t)blocks;
    blocks += (uint64_t)ceil_div(d.n, e.rows_per_tile);
    // the squared-sum entry: what opt_plan makes of the gradient of a contiguous, aligned [n, cols] variable
    OptEntry q{};
    q.g = d.grad_rows;
    q.n = (uint32_t)numel;
    const bool contiguous = d.n == 1 || d.ld_grad == d.cols;
    q.cols = contiguous ? q.n : (uint32_t)d.cols;
    q.ldw = q.cols;
    q.ldg = contiguous ? q.n : (uint32_t)d.ld_grad;
    q.vec = opt_aligned(q.g) && (contiguous || (q.cols % 4 == 0 && q.ldg % 4 == 0));
    q.nparts = (uint32_t)ceil_div(numel, OPT_SUM_ELEMS);
    q.part0 = (uint32_t)plan.total_parts;
    plan.total_parts += q.nparts;
    e.part0 = q.part0;
    e.nparts = q.nparts;
    e.quad_elems = q.vec ? (q.n & ~3u) : 0u;
    rows.r.push_back(e);
    rows.sum.push_back(q);
  }
  TFGNN_REQUIRE(plan.total_parts < (1ull << 31) && blocks < (1ull << 31), "tfgnn_optimizer: too many elements");
  rows.blocks = (uint32_t)blocks;
  return TFGNN_OK;
}

static int opt_check_config(const tfgnn_opt_config* cfg) {
  TFGNN_REQUIRE(cfg != nullptr && cfg->struct_size == sizeof(tfgnn_opt_config),
                "tfgnn_optimizer_apply: config missing or of another size (struct_size %zu, expected %zu)",
                cfg ? cfg->struct_size : (size_t)0, sizeof(tfgnn_opt_config));
  const tfgnn_opt_config& c = *cfg;
  TFGNN_REQUIRE(c.kind >= TFGNN_OPT_SGD && c.kind <= TFGNN_OPT_ADAM, "tfgnn_optimizer_apply: unknown optimizer kind %d", c.kind);
  TFGNN_REQUIRE(c.clip >= TFGNN_CLIP_NONE && c.clip <= TFGNN_CLIP_GLOBAL_NORM, "tfgnn_optimizer_apply: unknown clip mode %d", c.clip);
  TFGNN_REQUIRE(c.clip == TFGNN_CLIP_NONE || (std::isfinite(c.clip_value) && c.clip_value > 0.f),
                "tfgnn_optimizer_apply: clip value %g must be positive and finite", (double)c.clip_value);
  TFGNN_REQUIRE(c.momentum >= 0.f && c.momentum <= 1.f, "tfgnn_optimizer_apply: momentum %g outside [0, 1]", (double)c.momentum);
  TFGNN_REQUIRE(c.schedule == 0 || c.schedule == 1, "tfgnn_optimizer_apply: unknown schedule %d", c.schedule);
  TFGNN_REQUIRE(c.state != nullptr && opt_aligned(c.state), "tfgnn_optimizer_apply: NULL or unaligned state");
  return TFGNN_OK;
}

static int opt_check_workspace(const tfgnn_opt_config& c, size_t ws) {
  TFGNN_REQUIRE(ws == 0 || (c.workspace && opt_aligned(c.workspace) && c.workspace_bytes >= ws),
                "tfgnn_optimizer_apply: the norm modes need a 16-byte aligned workspace of %zu bytes (got %zu)", ws,
                c.workspace ? c.workspace_bytes : (size_t)0);
  return TFGNN_OK;
}

static int opt_kernel_kind(const tfgnn_opt_config& c) {
  if (c.kind == TFGNN_OPT_SGD) return c.momentum > 0.f ? OPT_K_SGD_MOM : OPT_K_SGD;
  if (c.kind == TFGNN_OPT_RMSPROP) return c.momentum > 0.f ? OPT_K_RMS_MOM : OPT_K_RMS;
  return OPT_K_ADAM;
}

static void opt_fill_params(const tfgnn_opt_config& c, const OptPlan& plan, OptParams& p) {
  p.kind = c.kind;
  p.clip = c.clip;
  p.clip_value = c.clip_value;
  p.momentum = c.momentum;
  p.rho = c.rho;
  p.beta_1 = c.beta_1;
  p.beta_2 = c.beta_2;
  p.epsilon = c.epsilon;
  p.schedule = c.schedule;
  p.lr = c.learning_rate;
  p.lr_initial = c.initial_learning_rate;
  p.lr_final = c.final_learning_rate;
  p.power = c.power;
  p.warmup = (float)c.warmup_steps;
  p.decay = (float)c.decay_steps;
  p.state = (unsigned long long*)c.state;
  p.partials = (double*)c.workspace;
  p.total_parts = (uint32_t)plan.total_parts;
}

// the launches of the dense tensors: with `sums` the squared-sum pass first (the row tensors' entries `row_sums` ride in the
// launch of the last chunk, or have one of their own when there is no dense tensor), then the update, one launch per chunk;
// the last update launch takes the ticket when `advance`
static int opt_launch_dense(const OptPlan& plan, const std::vector<OptEntry>* row_sums, OptTable& tab, int kk, bool sums,
                            bool advance, hipStream_t s) {
  OptParams& p = tab.p;
  const size_t ne = plan.e.size(), nr = row_sums ? row_sums->size() : 0;
  for (int phase = sums ? 0 : 1; phase < 2; ++phase) {
    for (size_t first = 0; first < ne || (phase == 0 && first == 0 && nr); first += OPT_CHUNK) {
      const size_t last = std::min(ne, first + OPT_CHUNK);
      p.n = (int)(last - first);
      uint32_t blocks = 0;
      for (size_t i = first; i < last; ++i) {
        tab.e[i - first] = plan.e[i];
        tab.e[i - first].blk0 = blocks;
        blocks += phase == 0 ? plan.e[i].nparts : plan.upd_blocks[i];
      }
      p.part_base = first < ne ? plan.e[first].part0 : 0;
      p.advance = phase == 1 && last == ne && advance;
      if (phase == 0 && last == ne && nr) {
        OptSumRowsTable big{};
        for (size_t i = 0; i < last - first; ++i) big.e[i] = tab.e[i];
        for (size_t i = 0; i < nr; ++i) {
          big.e[last - first + i] = (*row_sums)[i];
          blocks += (*row_sums)[i].nparts;
        }
        if (first == ne) p.part_base = (*row_sums)[0].part0;
        p.n += (int)nr;
        p.blocks = blocks;
        big.p = p;
        hipLaunchKernelGGL(opt_sumsq_rows_kernel, dim3(blocks), dim3(OPT_THREADS), 0, s, big);
      } else if (phase == 0) {
        p.blocks = blocks;
        hipLaunchKernelGGL(opt_sumsq_kernel, dim3(blocks), dim3(OPT_THREADS), 0, s, tab);
      } else {
        p.blocks = blocks;
        switch (kk) {
          case OPT_K_SGD: hipLaunchKernelGGL(opt_update_kernel<OPT_K_SGD>, dim3(blocks), dim3(OPT_THREADS), 0, s, tab); break;
          case OPT_K_SGD_MOM: hipLaunchKernelGGL(opt_update_kernel<OPT_K_SGD_MOM>, dim3(blocks), dim3(OPT_THREADS), 0, s, tab); break;
          case OPT_K_RMS: hipLaunchKernelGGL(opt_update_kernel<OPT_K_RMS>, dim3(blocks), dim3(OPT_THREADS), 0, s, tab); break;
          case OPT_K_RMS_MOM: hipLaunchKernelGGL(opt_update_kernel<OPT_K_RMS_MOM>, dim3(blocks), dim3(OPT_THREADS), 0, s, tab); break;
          default: hipLaunchKernelGGL(opt_update_kernel<OPT_K_ADAM>, dim3(blocks), dim3(OPT_THREADS), 0, s, tab); break;
        }
      }
      TFGNN_LAUNCH_CHECK();
      g_opt_launches.fetch_add(1, std::memory_order_relaxed);
    }
  }
  return TFGNN_OK;
}

}  // namespace tfgnn

extern "C" size_t tfgnn_optimizer_workspace_bytes(const tfgnn_opt_tensor* tensors, int n, int clip) {
  using namespace tfgnn;
  OptPlan plan;
  if (opt_plan(tensors, n, TFGNN_OPT_SGD, 0.f, plan) != TFGNN_OK) return 0;
  return opt_workspace_bytes(plan, clip);
}

extern "C" int tfgnn_optimizer_apply(const tfgnn_opt_tensor* tensors, int n, const tfgnn_opt_config* cfg, void* stream) {
  using namespace tfgnn;
  int st = opt_check_config(cfg);
  if (st != TFGNN_OK) return st;
  const tfgnn_opt_config& c = *cfg;
  OptPlan plan;
  st = opt_plan(tensors, n, c.kind, c.momentum, plan);
  if (st != TFGNN_OK) return st;
  TFGNN_REQUIRE(!plan.e.empty(), "tfgnn_optimizer_apply: no elements to update");
  const size_t ws = opt_workspace_bytes(plan, c.clip);
  st = opt_check_workspace(c, ws);
  if (st != TFGNN_OK) return st;
  OptTable tab{};
  opt_fill_params(c, plan, tab.p);
  return opt_launch_dense(plan, nullptr, tab, opt_kernel_kind(c), ws != 0, true, (hipStream_t)stream);
}

extern "C" size_t tfgnn_optimizer_rows_workspace_bytes(const tfgnn_opt_tensor* tensors, int n, const tfgnn_opt_row_tensor* row_tensors,
                                                       int n_rows, int clip) {
  using namespace tfgnn;
  OptPlan plan;
  OptRowPlan rows;
  if (opt_plan(tensors, n, TFGNN_OPT_SGD, 0.f, plan) != TFGNN_OK) return 0;
  if (opt_plan_rows(row_tensors, n_rows, TFGNN_OPT_SGD, 0.f, plan, rows) != TFGNN_OK) return 0;
  return opt_workspace_bytes(plan, clip);
}

extern "C" int tfgnn_optimizer_apply_rows(const tfgnn_opt_tensor* tensors, int n, const tfgnn_opt_row_tensor* row_tensors, int n_rows,
                                          const tfgnn_opt_config* cfg, void* stream) {
  using namespace tfgnn;
  int st = opt_check_config(cfg);
  if (st != TFGNN_OK) return st;
  const tfgnn_opt_config& c = *cfg;
  OptPlan plan;
  OptRowPlan rows;
  st = opt_plan(tensors, n, c.kind, c.momentum, plan);
  if (st != TFGNN_OK) return st;
  st = opt_plan_rows(row_tensors, n_rows, c.kind, c.momentum, plan, rows);
  if (st != TFGNN_OK) return st;
  const size_t ws = opt_workspace_bytes(plan, c.clip);
  st = opt_check_workspace(c, ws);
  if (st != TFGNN_OK) return st;
  const int kk = opt_kernel_kind(c);
  const hipStream_t s = (hipStream_t)stream;
  // the row launch is the call's last and takes the ticket; without a row to update the last dense launch keeps it, and a call
  // with nothing at all to update advances the counter with one workgroup of the row launch
  const bool row_launch = rows.blocks > 0 || plan.e.empty();
  OptTable tab{};
  opt_fill_params(c, plan, tab.p);
  st = opt_launch_dense(plan, &rows.sum, tab, kk, ws != 0, !row_launch, s);
  if (st != TFGNN_OK || !row_launch) return st;
  OptRowTable rt{};
  rt.p = tab.p;
  rt.p.n = (int)rows.r.size();
  rt.p.part_base = 0;
  rt.p.blocks = std::max(rows.blocks, 1u);
  rt.p.advance = 1;
  for (size_t i = 0; i < rows.r.size(); ++i) rt.r[i] = rows.r[i];
  const dim3 grid(rt.p.blocks), block(OPT_THREADS);
  switch (kk) {
    case OPT_K_SGD: hipLaunchKernelGGL(opt_update_rows_kernel<OPT_K_SGD>, grid, block, 0, s, rt); break;
    case OPT_K_SGD_MOM: hipLaunchKernelGGL(opt_update_rows_kernel<OPT_K_SGD_MOM>, grid, block, 0, s, rt); break;
    case OPT_K_RMS: hipLaunchKernelGGL(opt_update_rows_kernel<OPT_K_RMS>, grid, block, 0, s, rt); break;
    case OPT_K_RMS_MOM: hipLaunchKernelGGL(opt_update_rows_kernel<OPT_K_RMS_MOM>, grid, block, 0, s, rt); break;
    default: hipLaunchKernelGGL(opt_update_rows_kernel<OPT_K_ADAM>, grid, block, 0, s, rt); break;
  }
  TFGNN_LAUNCH_CHECK();
  g_opt_launches.fetch_add(1, std::memory_order_relaxed);
  return TFGNN_OK;
}

extern "C" int tfgnn_optimizer_iterations_get(const int64_t* state, int64_t* out, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(state && out, "tfgnn_optimizer_iterations_get: NULL pointer");
  hipLaunchKernelGGL(opt_iterations_get_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (const long long*)state, (long long*)out);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}

extern "C" int tfgnn_optimizer_iterations_set(int64_t* state, int64_t value, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(state, "tfgnn_optimizer_iterations_set: NULL state");
  TFGNN_REQUIRE(value >= 0, "tfgnn_optimizer_iterations_set: negative step %lld", (long long)value);
  hipLaunchKernelGGL(opt_iterations_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)state, (long long)value);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}

extern "C" int64_t tfgnn_optimizer_launch_count(void) { return tfgnn::g_opt_launches.load(std::memory_order_relaxed); }
