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

typedef const __attribute__((address_space(4))) OptTable* opt_table_cptr;
typedef const __attribute__((address_space(4))) OptEntry* opt_entry_cptr;

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
__global__ void __launch_bounds__(OPT_THREADS) opt_sumsq_kernel(OptTable table) {
  (void)table;
  __shared__ double red[OPT_THREADS / 64];
  const opt_table_cptr T = opt_table();
  const uint32_t b = T->p.part_base + blockIdx.x;
  int k = 0;
  const int n_t = T->p.n;
  while (k + 1 < n_t && b >= T->e[k + 1].part0) ++k;
  const opt_entry_cptr E = &T->e[k];
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
  if (threadIdx.x == 0) T->p.partials[b] = s;
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
__device__ __forceinline__ float opt_learning_rate(opt_table_cptr T, float step) {
  const float lr = T->p.lr;
  if (!T->p.schedule) return lr;
  const float warmup = T->p.warmup, decay = T->p.decay, power = T->p.power;
  if (step <= warmup) return (lr - T->p.lr_initial) * powf(step / warmup, power) + T->p.lr_initial;
  const float s = fminf(step - warmup, decay);
  return (lr - T->p.lr_final) * powf(1.f - s / decay, power) + T->p.lr_final;
}

// sum of partials[lo, hi) in a fixed order: every workgroup of a tensor (or of the call) computes the same bits
__device__ __forceinline__ double opt_sum_partials(const double* __restrict__ p, uint32_t lo, uint32_t hi, double* red) {
  double acc = 0.0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += OPT_THREADS) acc += p[i];
  return opt_block_sum(acc, red);
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
  OptCoef c;
  c.lr = opt_learning_rate(T, (float)it);
  c.mu = T->p.momentum;
  c.rho = T->p.rho;
  c.one_minus_rho = 1.f - T->p.rho;
  c.eps = T->p.epsilon;
  c.one_minus_b1 = 1.f - T->p.beta_1;
  c.one_minus_b2 = 1.f - T->p.beta_2;
  if (KIND == OPT_K_ADAM) {
    const float t = (float)(it + 1);
    const float b1p = powf(T->p.beta_1, t), b2p = powf(T->p.beta_2, t);
    c.lr = c.lr * (sqrtf(1.f - b2p) / (1.f - b1p));
  }
  c.clip = T->p.clip;
  c.c = T->p.clip_value;
  c.den = 1.f;
  c.scale = 1.f;
  if (c.clip == TFGNN_CLIP_NORM) {
    const float norm = (float)sqrt(opt_sum_partials(T->p.partials, E->part0, E->part0 + E->nparts, red));
    c.den = fmaxf(norm, c.c);
  } else if (c.clip == TFGNN_CLIP_GLOBAL_NORM) {
    const float norm = (float)sqrt(opt_sum_partials(T->p.partials, 0, T->p.total_parts, red));
    // clip_by_global_norm: clip_norm * minimum(1 / use_norm, 1 / clip_norm), NaN when the norm is not finite
    c.scale = isfinite(norm) ? c.c * fminf(1.f / norm, 1.f / c.c) : __builtin_nanf("");
  }

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

  if (T->p.advance) {
    // the ticket: the workgroup that arrives last has seen every other one read the counter and advances it; it resets the
    // ticket for the next call.  Relaxed: what orders a workgroup's read of the counter before its add is that thread 0 has
    // consumed the value (LDS store + barrier above); the update's own stores need no ordering (the next reader is another
    // launch), and a release here would write the L2 back once per workgroup (buffer_wbl2; measured: it doubled the call's time).
    if (threadIdx.x == 0) {
      unsigned long long* st = T->p.state;
      const unsigned long long t = __hip_atomic_fetch_add(st + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t == (unsigned long long)T->p.blocks - 1) {
        __hip_atomic_store(st + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st, it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
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

}  // namespace tfgnn

extern "C" size_t tfgnn_optimizer_workspace_bytes(const tfgnn_opt_tensor* tensors, int n, int clip) {
  using namespace tfgnn;
  OptPlan plan;
  if (opt_plan(tensors, n, TFGNN_OPT_SGD, 0.f, plan) != TFGNN_OK) return 0;
  return opt_workspace_bytes(plan, clip);
}

extern "C" int tfgnn_optimizer_apply(const tfgnn_opt_tensor* tensors, int n, const tfgnn_opt_config* cfg, void* stream) {
  using namespace tfgnn;
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
  OptPlan plan;
  const int st = opt_plan(tensors, n, c.kind, c.momentum, plan);
  if (st != TFGNN_OK) return st;
  TFGNN_REQUIRE(!plan.e.empty(), "tfgnn_optimizer_apply: no elements to update");
  const size_t ws = opt_workspace_bytes(plan, c.clip);
  TFGNN_REQUIRE(ws == 0 || (c.workspace && opt_aligned(c.workspace) && c.workspace_bytes >= ws),
                "tfgnn_optimizer_apply: the norm modes need a 16-byte aligned workspace of %zu bytes (got %zu)", ws,
                c.workspace ? c.workspace_bytes : (size_t)0);

  int kk;
  if (c.kind == TFGNN_OPT_SGD) kk = c.momentum > 0.f ? OPT_K_SGD_MOM : OPT_K_SGD;
  else if (c.kind == TFGNN_OPT_RMSPROP) kk = c.momentum > 0.f ? OPT_K_RMS_MOM : OPT_K_RMS;
  else kk = OPT_K_ADAM;

  OptTable tab{};
  OptParams& p = tab.p;
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

  const size_t ne = plan.e.size();
  const hipStream_t s = (hipStream_t)stream;
  for (int phase = ws ? 0 : 1; phase < 2; ++phase) {
    for (size_t first = 0; first < ne; first += OPT_CHUNK) {
      const size_t last = std::min(ne, first + OPT_CHUNK);
      p.n = (int)(last - first);
      uint32_t blocks = 0;
      for (size_t i = first; i < last; ++i) {
        tab.e[i - first] = plan.e[i];
        tab.e[i - first].blk0 = blocks;
        blocks += phase == 0 ? plan.e[i].nparts : plan.upd_blocks[i];
      }
      p.part_base = plan.e[first].part0;
      p.blocks = blocks;
      p.advance = phase == 1 && last == ne;
      if (phase == 0) {
        hipLaunchKernelGGL(opt_sumsq_kernel, dim3(blocks), dim3(OPT_THREADS), 0, s, tab);
      } else {
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
