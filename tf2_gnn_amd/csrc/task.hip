// Task metrics at the end of the path: the losses the reference differentiates and the
// numbers its epoch loop aggregates.
//   tfgnn_sigmoid_ce_metrics: NodeMulticlassTask._fast_task_metrics + micro_f1 (tf2_gnn/models/node_multiclass_task.py:10-23,62-70)
//   tfgnn_regression_metrics: tf.losses.mean_squared_error / mean_absolute_error of the per-graph outputs
//                             (tf2_gnn/models/graph_regression_task.py:157-158, tf2_gnn/models/qm9_regression.py:122-123)
//   tfgnn_binary_ce_metrics:  GraphBinaryClassificationTask.compute_task_metrics on the per-graph LOGITS
//                             (tf2_gnn/models/graph_binary_classification_task.py:31-58): sigmoid, binary cross-entropy of the
//                             probabilities, accuracy counts, d loss / d logit
//   tfgnn_softmax_ce_metrics: no reference counterpart (NodeClassificationTask): weighted softmax cross-entropy of per-node
//                             logits against one class per node, accuracy counts, argmax, d loss / d logits; the contract is
//                             the comment in include/tfgnn.h
// All are one streaming pass (HBM-bound, 8 - 20 bytes per element) with a two-stage, fixed-order reduction: stage 1 leaves
// one partial per workgroup, stage 2 (one workgroup) adds them in index order, so the loss is reproducible run to run.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"

namespace tfgnn {

constexpr int TASK_BLOCKS = 1024;

struct TaskPartial {
  double a;              // CE, binary CE, softmax CE: sum of element losses | regression: sum of squared errors
  double b;              // regression: sum of absolute errors | softmax CE: sum of the counted nodes' weights
  long long tp, fp, fn;  // CE: micro-F1 counts | binary CE: confusion counts (tn = G - tp - fp - fn)
                         // softmax CE: tp = correct, fp = counted
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void block_reduce_store(TaskPartial mine, TaskPartial* out) {
  __shared__ TaskPartial sh[4];
  mine.a = wave_sum(mine.a);
  mine.b = wave_sum(mine.b);
  mine.tp = wave_sum(mine.tp);
  mine.fp = wave_sum(mine.fp);
  mine.fn = wave_sum(mine.fn);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    TaskPartial t = sh[0];
    for (int w = 1; w < 4; ++w) {
      t.a += sh[w].a; t.b += sh[w].b; t.tp += sh[w].tp; t.fp += sh[w].fp; t.fn += sh[w].fn;
    }
    *out = t;
  }
}

// element (v, c): x = logits, z = labels.
//   loss  max(x, 0) - x z + log1p(exp(-|x|))            [ext] tf.nn.sigmoid_cross_entropy_with_logits
//   pred  round(sigmoid(x)) as int32, label int32(z)     node_multiclass_task.py:12-14
//   grad  (sigmoid(x) - z) / V                           d mean_v(sum_c loss) / dx
__global__ void __launch_bounds__(256)
sigmoid_ce_partial_kernel(const float* __restrict__ logits, int64_t ld_x, const float* __restrict__ labels, int64_t ld_z,
                          int64_t V, int64_t C, float inv_v, float* __restrict__ dlogits, TaskPartial* __restrict__ partials) {
  TaskPartial mine = {0.0, 0.0, 0, 0, 0};
  const int64_t total = V * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / C, c = i - v * C;
    const float x = logits[v * ld_x + c], z = labels[v * ld_z + c];
    mine.a += (double)(fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x))));
    const float p = 1.0f / (1.0f + expf(-x));
    const int pred = (int)rintf(p), lab = (int)z;
    mine.tp += (pred * lab) != 0;
    mine.fp += (pred * (lab - 1)) != 0;
    mine.fn += ((pred - 1) * lab) != 0;
    if (dlogits) dlogits[i] = (p - z) * inv_v;
  }
  block_reduce_store(mine, partials + blockIdx.x);
}

__global__ void __launch_bounds__(256)
regression_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t G, float two_over_g,
                          float* __restrict__ dpred, TaskPartial* __restrict__ partials) {
  TaskPartial mine = {0.0, 0.0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = pred[i] - target[i];
    mine.a += (double)d * d;
    mine.b += (double)fabsf(d);
    if (dpred) dpred[i] = two_over_g * d;  // d mse / d pred
  }
  block_reduce_store(mine, partials + blockIdx.x);
}

// graph g: x = logit, y = target (0 / 1).  [ext] tf.keras.losses.binary_crossentropy(from_logits=False) as the Keras backend
// writes it for a probability input - clip to [eps, 1 - eps], then "+ eps" inside both logs - on p = sigmoid(x), eps =
// K.epsilon() = float32(1e-7), hi = float32(1) - eps (PARITY UNPINNED: TensorFlow cannot run beside this library).  Some TF
// versions, inside tf.function, recognise the Sigmoid producer of y_pred and evaluate the logits form instead; the two differ
// only where p is clipped.
//   p     sigmoid(x);  pc = min(max(p, eps), hi)
//   loss  -( y log(pc + eps) + (1 - y) log(1 - pc + eps) )
//   pred  rint(p): round half to even (tf.math.round), a logit of exactly 0 predicts 0; correct where pred == y as floats
//   grad  ( -(y / (pc + eps)) + (1 - y) / (1 - pc + eps) ) p (1 - p) / G  where eps <= p <= hi, 0 outside (clip_by_value)
// 1 - p is evaluated as sigmoid(-x), not as the fp32 difference: at |x| = 12 the difference keeps 7 bits (1 - p = 6e-6 next
// to a spacing of 6e-8 below 1), which would put an error of 1e-2 on a log of 12.  Inside the clip range 1 - pc IS 1 - p; at
// the two clip values it is the fp32 difference the formula states (1 - hi = 2^-23 exactly).
__global__ void __launch_bounds__(256)
binary_ce_partial_kernel(const float* __restrict__ logits, const float* __restrict__ target, int64_t G, float inv_g,
                         float* __restrict__ prob, float* __restrict__ dlogits, TaskPartial* __restrict__ partials) {
  TaskPartial mine = {0.0, 0.0, 0, 0, 0};
  const float eps = 1e-7f, hi = 1.0f - eps;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = logits[i], y = target[i];
    const float p = 1.0f / (1.0f + expf(-x)), q = 1.0f / (1.0f + expf(x));  // q = 1 - p
    const bool inside = p >= eps && p <= hi;
    const float pc = fminf(fmaxf(p, eps), hi);
    const float qc = inside ? q : 1.0f - pc;
    const float a = pc + eps, b = qc + eps;
    mine.a -= (double)(y * logf(a) + (1.0f - y) * logf(b));
    const float pred = rintf(p);
    // every graph lands in exactly one of the four; tp + tn = number of pred == y also for a target that is not 0 / 1
    mine.tp += pred == 1.0f && y == 1.0f;
    mine.fp += pred == 1.0f && y != 1.0f;
    mine.fn += pred == 0.0f && y != 0.0f;
    if (prob) prob[i] = p;
    if (dlogits) dlogits[i] = inside ? ((1.0f - y) / b - y / a) * (p * q) * inv_g : 0.0f;
  }
  block_reduce_store(mine, partials + blockIdx.x);
}

// ---- softmax cross-entropy (include/tfgnn.h tfgnn_softmax_ce_metrics) --------------------------------------------------------
constexpr int SOFTMAX_CE_BLOCKS = 2048;       // main pass: 8 workgroups of 4 waves per CU, every wave slot of the part taken
constexpr int SOFTMAX_CE_WEIGHT_BLOCKS = 64;  // partials of the weight pre-pass: one per lane of the wave that adds them up
constexpr int SOFTMAX_CE_REGS = 8;            // logits a lane keeps in registers; a row of C <= 8 * 64 is read once

// node v is counted iff its weight is > 0 and its label an integer in [0, C); NaN fails both comparisons
__device__ __forceinline__ bool softmax_ce_counted(float y, float w, int64_t C) {
  return w > 0.0f && y >= 0.0f && y < (float)C && y == floorf(y);
}

// Stage 0: the weight sum W and the number of counted nodes, one partial per workgroup (b, fp).
__global__ void __launch_bounds__(256)
softmax_ce_weight_kernel(const float* __restrict__ labels, int64_t ld_y, const float* __restrict__ weights, int64_t ld_w,
                         int64_t V, int64_t C, TaskPartial* __restrict__ partials) {
  TaskPartial mine = {0.0, 0.0, 0, 0, 0};
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const float w = weights ? weights[v * ld_w] : 1.0f;
    if (softmax_ce_counted(labels[v * ld_y], w, C)) {
      mine.b += (double)w;
      mine.fp += 1;
    }
  }
  block_reduce_store(mine, partials + blockIdx.x);
}

// (value, index) of the maximum over the G lanes of a group, the lowest index among equal values; every lane gets it
template <int G>
__device__ __forceinline__ void group_argmax(float& m, int& idx) {
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o);
    const int oi = __shfl_xor(idx, o);
    if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
  }
}
template <int G>
__device__ __forceinline__ float group_sum(float s) {
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

// Stage 1.  A wave holds 64 / G rows at a time, G lanes per row, lane j of a group the columns j, j + G, j + 2 G, ...:
// consecutive lanes read consecutive columns, and the groups of a wave consecutive rows.  STREAM == false: the row sits in
// SOFTMAX_CE_REGS registers per lane and is read once.  STREAM == true (G = 64): running maximum and rescaled sum per lane,
// merged across the wave; the gradient reads the row a second time.  A NaN never wins the maximum (it counts as -inf there)
// and poisons the sum.  Rows go to waves in a fixed grid-stride order, lane 0 of a group carries the row's terms, and
// block_reduce_store adds them in a fixed tree: the partials are the same bits whether or not dlogits / pred are written.
template <int G, bool STREAM>
__global__ void __launch_bounds__(256)
softmax_ce_partial_kernel(const float* __restrict__ logits, int64_t ld_x, const float* __restrict__ labels, int64_t ld_y,
                          const float* __restrict__ weights, int64_t ld_w, int64_t V, int64_t C,
                          const TaskPartial* __restrict__ weight_partials, int num_weight_partials,
                          float* __restrict__ dlogits, int64_t ld_d, int32_t* __restrict__ pred,
                          TaskPartial* __restrict__ partials) {
  constexpr int ROWS = 64 / G;  // rows per wave and step
  const int lane = threadIdx.x & 63, sub = lane % G;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), num_waves = (int64_t)gridDim.x * 4;
  // W: the pre-pass partials, one per lane, added in the butterfly's fixed order - every lane of every wave gets the same bits
  const double W = wave_sum(lane < num_weight_partials ? weight_partials[lane].b : 0.0);
  const float neg_inf = -INFINITY;
  TaskPartial mine = {0.0, 0.0, 0, 0, 0};
  for (int64_t v0 = wave * ROWS; v0 < V; v0 += num_waves * ROWS) {  // wave-uniform trip count: the shuffles need all lanes
    const int64_t v = v0 + lane / G;
    const bool live = v < V;
    const float* row = logits + (live ? v : 0) * ld_x;
    float x[SOFTMAX_CE_REGS];
    float m = neg_inf, s = 0.0f;
    int best = INT_MAX;
    if constexpr (!STREAM) {
#pragma unroll
      for (int k = 0; k < SOFTMAX_CE_REGS; ++k) {
        const int c = k * G + sub;
        x[k] = (live && c < C) ? row[c] : neg_inf;
      }
#pragma unroll
      for (int k = 0; k < SOFTMAX_CE_REGS; ++k) {  // ascending columns: a strict > keeps the lowest index
        const int c = k * G + sub;
        const float xv = x[k] != x[k] ? neg_inf : x[k];
        if (c < C && (xv > m || best == INT_MAX)) { m = xv; best = c; }
      }
      group_argmax<G>(m, best);
#pragma unroll
      for (int k = 0; k < SOFTMAX_CE_REGS; ++k) {
        const int c = k * G + sub;
        x[k] = expf(x[k] - m);  // the gradient reuses the exponentials
        if (c < C) s += x[k];
      }
      s = group_sum<G>(s);
    } else {
      if (live) {
        for (int64_t c = sub; c < C; c += G) {
          const float xc = row[c];
          const float xv = xc != xc ? neg_inf : xc;
          if (xv > m || best == INT_MAX) {
            s = (m == xv) ? s : s * expf(m - xv);  // m == xv only at -inf, where s is still 0 or NaN
            m = xv;
            best = (int)c;
          }
          s += (xc == neg_inf && m == neg_inf) ? 0.0f : expf(xc - m);
        }
      }
      const float lane_m = m;
      group_argmax<G>(m, best);
      s = (lane_m == m) ? s : s * expf(lane_m - m);
      s = group_sum<G>(s);
    }
    if (!live) continue;  // after the last shuffle of the step
    const float y = labels[v * ld_y], w = weights ? weights[v * ld_w] : 1.0f;
    const bool counted = softmax_ce_counted(y, w, C);
    const int label = counted ? (int)y : -1;
    if (sub == 0) {
      if (pred) pred[v] = best;
      if (counted) {
        mine.a += (double)w * ((double)m - (double)row[label] + (double)logf(s));
        mine.tp += best == label;
      }
    }
    if (dlogits) {
      float* drow = dlogits + v * ld_d;
      const float scale = counted ? (float)((double)w / W) : 0.0f;
      if constexpr (!STREAM) {
#pragma unroll
        for (int k = 0; k < SOFTMAX_CE_REGS; ++k) {
          const int c = k * G + sub;
          if (c < C) drow[c] = counted ? scale * (x[k] / s - (c == label ? 1.0f : 0.0f)) : 0.0f;
        }
      } else {
        for (int64_t c = sub; c < C; c += G)
          drow[c] = counted ? scale * (expf(row[c] - m) / s - (c == label ? 1.0f : 0.0f)) : 0.0f;
      }
    }
  }
  block_reduce_store(mine, partials + blockIdx.x);
}

// kind 0: metrics = {mean per-node loss, micro-F1}, counts = {tp, fp, fn};  kind 1: metrics = {mse, mae};
// kind 2: metrics = {mean loss, accuracy}, counts = {tp, fp, tn, fn} (denom = G, an integer)
// kind 3: softmax CE; the partials are those of the main pass (a, tp) followed by those of the weight pre-pass (b, fp):
//         metrics = {a / b, or 0 when no node is counted; tp / fp, 0 / 0 -> nan}, counts = {tp, fp}
__global__ void __launch_bounds__(256)
task_final_kernel(const TaskPartial* __restrict__ partials, int n, int kind, double denom, float* __restrict__ metrics,
                  long long* __restrict__ counts) {
  TaskPartial mine = {0.0, 0.0, 0, 0, 0};
  // fixed order: thread t adds partials t, t+256, ...; the tree over threads is fixed as well
  for (int i = threadIdx.x; i < n; i += 256) {
    const TaskPartial p = partials[i];
    mine.a += p.a; mine.b += p.b; mine.tp += p.tp; mine.fp += p.fp; mine.fn += p.fn;
  }
  __shared__ TaskPartial total;
  block_reduce_store(mine, &total);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (kind == 0) {
      metrics[0] = (float)(total.a / denom);
      // int64 / int64 -> float64 in the reference (node_multiclass_task.py:20-23); 0/0 -> nan as there
      const double tp = (double)total.tp, fp = (double)total.fp, fn = (double)total.fn;
      const double precision = tp / (tp + fp), recall = tp / (tp + fn);
      metrics[1] = (float)((2.0 * precision * recall) / (precision + recall));
      if (counts) { counts[0] = total.tp; counts[1] = total.fp; counts[2] = total.fn; }
    } else if (kind == 1) {
      metrics[0] = (float)(total.a / denom);
      metrics[1] = (float)(total.b / denom);
    } else if (kind == 2) {
      const long long tn = (long long)denom - total.tp - total.fp - total.fn;
      metrics[0] = (float)(total.a / denom);
      metrics[1] = (float)((double)(total.tp + tn) / denom);
      if (counts) { counts[0] = total.tp; counts[1] = total.fp; counts[2] = tn; counts[3] = total.fn; }
    } else {
      metrics[0] = total.fp > 0 ? (float)(total.a / total.b) : 0.0f;
      metrics[1] = (float)((double)total.tp / (double)total.fp);
      if (counts) { counts[0] = total.tp; counts[1] = total.fp; }
    }
  }
}

static int task_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(TASK_BLOCKS, ceil_div(n, 256 * 4))); }

}  // namespace tfgnn

extern "C" size_t tfgnn_task_metrics_workspace_bytes(void) { return sizeof(tfgnn::TaskPartial) * tfgnn::TASK_BLOCKS; }

extern "C" int tfgnn_sigmoid_ce_metrics(const float* d_logits, int64_t ld_logits, const float* d_labels, int64_t ld_labels,
                                        int64_t V, int64_t C, float* d_metrics, int64_t* d_counts, float* d_dlogits,
                                        void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(V > 0 && C > 0, "sigmoid_ce_metrics: empty batch (the reference's reduce_mean gives nan)");
  TFGNN_REQUIRE(d_logits && d_labels && d_metrics, "NULL pointer");
  TFGNN_REQUIRE(ld_logits >= C && ld_labels >= C, "bad leading dimension");
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= tfgnn_task_metrics_workspace_bytes() && (uintptr_t)d_workspace % 8 == 0,
                "workspace of tfgnn_task_metrics_workspace_bytes() bytes required");
  hipStream_t s = (hipStream_t)stream;
  TaskPartial* partials = (TaskPartial*)d_workspace;
  const int grid = task_grid(V * C);
  hipLaunchKernelGGL(sigmoid_ce_partial_kernel, dim3(grid), dim3(256), 0, s, d_logits, ld_logits, d_labels, ld_labels, V, C,
                     1.0f / (float)V, d_dlogits, partials);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(task_final_kernel, dim3(1), dim3(256), 0, s, partials, grid, 0, (double)V, d_metrics, (long long*)d_counts);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}

extern "C" int tfgnn_regression_metrics(const float* d_pred, const float* d_target, int64_t G, float* d_metrics, float* d_dpred,
                                        void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(G > 0, "regression_metrics: empty batch (the reference's mean gives nan)");
  TFGNN_REQUIRE(d_pred && d_target && d_metrics, "NULL pointer");
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= tfgnn_task_metrics_workspace_bytes() && (uintptr_t)d_workspace % 8 == 0,
                "workspace of tfgnn_task_metrics_workspace_bytes() bytes required");
  hipStream_t s = (hipStream_t)stream;
  TaskPartial* partials = (TaskPartial*)d_workspace;
  const int grid = task_grid(G);
  hipLaunchKernelGGL(regression_partial_kernel, dim3(grid), dim3(256), 0, s, d_pred, d_target, G, 2.0f / (float)G, d_dpred, partials);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(task_final_kernel, dim3(1), dim3(256), 0, s, partials, grid, 1, (double)G, d_metrics, (long long*)nullptr);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}

extern "C" int tfgnn_binary_ce_metrics(const float* d_logits, const float* d_target, int64_t G, float* d_prob, float* d_metrics,
                                       int64_t* d_counts, float* d_dlogits, void* d_workspace, size_t workspace_bytes,
                                       void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(G > 0, "binary_ce_metrics: empty batch (the reference's reduce_mean gives nan)");
  TFGNN_REQUIRE(d_logits && d_target && d_metrics, "NULL pointer");
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= tfgnn_task_metrics_workspace_bytes() && (uintptr_t)d_workspace % 8 == 0,
                "workspace of tfgnn_task_metrics_workspace_bytes() bytes required");
  hipStream_t s = (hipStream_t)stream;
  TaskPartial* partials = (TaskPartial*)d_workspace;
  const int grid = task_grid(G);
  hipLaunchKernelGGL(binary_ce_partial_kernel, dim3(grid), dim3(256), 0, s, d_logits, d_target, G, 1.0f / (float)G, d_prob,
                     d_dlogits, partials);
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(task_final_kernel, dim3(1), dim3(256), 0, s, partials, grid, 2, (double)G, d_metrics, (long long*)d_counts);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}

extern "C" size_t tfgnn_softmax_ce_workspace_bytes(void) {
  return sizeof(tfgnn::TaskPartial) * (tfgnn::SOFTMAX_CE_BLOCKS + tfgnn::SOFTMAX_CE_WEIGHT_BLOCKS);
}

extern "C" int tfgnn_softmax_ce_metrics(const float* d_logits, int64_t ld_logits, const float* d_labels, int64_t ld_labels,
                                        const float* d_weights, int64_t ld_weights, int64_t V, int64_t C, float* d_metrics,
                                        int64_t* d_counts, float* d_dlogits, int64_t ld_dlogits, int32_t* d_pred,
                                        void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace tfgnn;
  TFGNN_REQUIRE(V > 0 && C > 0, "softmax_ce_metrics: empty batch (no node or no class)");
  TFGNN_REQUIRE(C <= ((int64_t)1 << 24), "softmax_ce_metrics: more than 2^24 classes (float32 labels stop being exact)");
  TFGNN_REQUIRE(d_logits && d_labels && d_metrics, "NULL pointer");
  TFGNN_REQUIRE(ld_logits >= C && ld_labels >= 1 && (!d_weights || ld_weights >= 1) && (!d_dlogits || ld_dlogits >= C),
                "bad leading dimension");
  TFGNN_REQUIRE(d_workspace && workspace_bytes >= tfgnn_softmax_ce_workspace_bytes() && (uintptr_t)d_workspace % 8 == 0,
                "workspace of tfgnn_softmax_ce_workspace_bytes() bytes required");
  hipStream_t s = (hipStream_t)stream;
  TaskPartial* partials = (TaskPartial*)d_workspace;
  // lane-group width: the smallest of 4, 8, 16, 32, 64 whose SOFTMAX_CE_REGS registers per lane hold the row
  int group = 4;
  while (group < 64 && (int64_t)group * SOFTMAX_CE_REGS < C) group *= 2;
  const bool stream_rows = C > 64 * SOFTMAX_CE_REGS;
  const int64_t waves = ceil_div(V, (int64_t)(64 / group));
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(SOFTMAX_CE_BLOCKS, ceil_div(waves, 4)));
  const int weight_grid = (int)std::max<int64_t>(1, std::min<int64_t>(SOFTMAX_CE_WEIGHT_BLOCKS, ceil_div(V, 256 * 4)));
  TaskPartial* weight_partials = partials + grid;  // behind the main pass's: task_final_kernel reads one array
  hipLaunchKernelGGL(softmax_ce_weight_kernel, dim3(weight_grid), dim3(256), 0, s, d_labels, ld_labels, d_weights, ld_weights, V,
                     C, weight_partials);
  TFGNN_LAUNCH_CHECK();
#define TFGNN_SOFTMAX_CE(G, STREAM)                                                                                         \
  hipLaunchKernelGGL((softmax_ce_partial_kernel<G, STREAM>), dim3(grid), dim3(256), 0, s, d_logits, ld_logits, d_labels,    \
                     ld_labels, d_weights, ld_weights, V, C, weight_partials, weight_grid, d_dlogits, ld_dlogits, d_pred, \
                     partials)
  if (stream_rows) TFGNN_SOFTMAX_CE(64, true);
  else if (group == 4) TFGNN_SOFTMAX_CE(4, false);
  else if (group == 8) TFGNN_SOFTMAX_CE(8, false);
  else if (group == 16) TFGNN_SOFTMAX_CE(16, false);
  else if (group == 32) TFGNN_SOFTMAX_CE(32, false);
  else TFGNN_SOFTMAX_CE(64, false);
#undef TFGNN_SOFTMAX_CE
  TFGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(task_final_kernel, dim3(1), dim3(256), 0, s, partials, grid + weight_grid, 3, 0.0, d_metrics,
                     (long long*)d_counts);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}
