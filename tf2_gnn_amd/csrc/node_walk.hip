// The second launch of the node-view walks (node_walk.hpp): rows made of several items.
#include "node_walk.hpp"

namespace tfgnn {
namespace {

// out[row, :] = ns[row] * (partial rows of the row added in item order)
__global__ void __launch_bounds__(256)
node_walk_combine_kernel(const int32_t* __restrict__ multi_row, const int32_t* __restrict__ multi_base, const int32_t* __restrict__ multi_n,
                         const float* __restrict__ partial, int width, const float* __restrict__ ns, float* __restrict__ out,
                         int64_t ld_out) {
  const int m = blockIdx.x;
  const int64_t row = multi_row[m];
  const int32_t base = multi_base[m], n = multi_n[m];
  const float scale = ns ? ns[row] : 1.f;
  for (int f = blockIdx.y * 256 + threadIdx.x; f < width; f += gridDim.y * 256) {
    float s = partial[(int64_t)base * width + f];
    for (int k = 1; k < n; ++k) s += partial[(int64_t)(base + k) * width + f];
    out[row * ld_out + f] = s * scale;
  }
}

}  // namespace

int node_walk_combine(const CsrPlan& p, const float* partial, int width, const float* ns, float* out, int64_t ld_out, hipStream_t s) {
  hipLaunchKernelGGL(node_walk_combine_kernel, dim3((unsigned)p.num_multi, (unsigned)std::min<int64_t>(ceil_div(width, 256), 64)), dim3(256),
                     0, s, p.multi_row, p.multi_base, p.multi_n, partial, width, ns, out, ld_out);
  TFGNN_LAUNCH_CHECK();
  return TFGNN_OK;
}

}  // namespace tfgnn
