// art_rebuild.hip -- gfx950 kernels of art_rebuild_device and art_get_tree_cost.
//
//   k_gather_tri9   one lane per triangle of the CLOSEST mesh (index order): the three corners are gathered from the caller's positions
//                   through the index triple into the 9-float layout the GPU builders read (build_bvh8_gpu's d_tri9).  Lanes below
//                   nverts count the bad vertices by the refit's rule (a coordinate not finite or beyond kRefitMaxCoord); the host reads
//                   the count before a builder starts, so a builder never sees such input.  New normals go through k_refit_tris
//                   (art_refit.hip), which rewrites the shading records.
//   k_tree_cost     one lane per node of the tree in HBM: the half surface areas of its child boxes (binary64, from the binary32 planes
//                   the walk tests), summed per kind of slot -- inner, leaf, leaf weighted by its triangle count -- by a wave reduction,
//                   a block reduction and one binary64 atomicAdd per block and sum.  The lane of node 0 also stores the area of the
//                   union of the root's used child boxes.  An empty slot adds nothing, nor does one a bad-vertex refit emptied (a plane
//                   that is not finite, or lo > hi).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "art_rebuild.h"
#include "art_refit.h"      // kRefitMaxCoord

namespace art {

constexpr int kGatherBlock = 256, kCostBlock = 256;

__global__ __launch_bounds__(kGatherBlock) void k_gather_tri9(const GatherArgs G) {
  const int64_t i = (int64_t)blockIdx.x * kGatherBlock + threadIdx.x;
  if (i < G.nverts) {
    const float* p = G.pos3f + 3 * i;
    if (!(fabsf(p[0]) <= kRefitMaxCoord && fabsf(p[1]) <= kRefitMaxCoord && fabsf(p[2]) <= kRefitMaxCoord)) atomicAdd(G.bad, 1ull);   // (false for NaN and +-inf)
  }
  if (i < G.n_prims) {
    float* t = G.tri9 + 9 * (size_t)i;
    for (int k = 0; k < 3; ++k) {
      const uint32_t v = (uint32_t)G.idx[3 * (size_t)i + k];
      const bool in = (int64_t)v < G.nverts;                              // (the upload checked the indices; never read outside pos3f)
      const float* s = G.pos3f + 3 * (size_t)(in ? v : 0u);
      t[3 * k] = in ? s[0] : 0.0f; t[3 * k + 1] = in ? s[1] : 0.0f; t[3 * k + 2] = in ? s[2] : 0.0f;
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

template <int W>
__global__ __launch_bounds__(kCostBlock) void k_tree_cost(const float* __restrict__ nodes, int n_nodes, double* __restrict__ out) {
  const int node = blockIdx.x * kCostBlock + threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0};                                          // inner slots | leaf slots | leaf slots x triangle count
  if (node < n_nodes) {
    const float* nd = nodes + (size_t)node * (8 * W);
    float ul[3] = {INFINITY, INFINITY, INFINITY}, uh[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int32_t ref = __float_as_int(nd[4 * j + 3]), cnt = __float_as_int(nd[4 * W + 4 * j + 3]);
      if (ref < 0) continue;
      const float l[3] = {nd[4 * j], nd[4 * j + 1], nd[4 * j + 2]}, h[3] = {nd[4 * W + 4 * j], nd[4 * W + 4 * j + 1], nd[4 * W + 4 * j + 2]};
      bool ok = true;
      for (int a = 0; a < 3; ++a) ok = ok && fabsf(l[a]) < INFINITY && fabsf(h[a]) < INFINITY && l[a] <= h[a];
      if (!ok) continue;
      const double dx = (double)h[0] - (double)l[0], dy = (double)h[1] - (double)l[1], dz = (double)h[2] - (double)l[2];
      const double A = dx * dy + dy * dz + dz * dx;
      if (cnt > 0) { s[1] += A; s[2] += (double)cnt * A; } else s[0] += A;
      for (int a = 0; a < 3; ++a) { ul[a] = fminf(ul[a], l[a]); uh[a] = fmaxf(uh[a], h[a]); }
    }
    if (node == 0 && ul[0] <= uh[0]) {
      const double dx = (double)uh[0] - (double)ul[0], dy = (double)uh[1] - (double)ul[1], dz = (double)uh[2] - (double)ul[2];
      out[3] = dx * dy + dy * dz + dz * dx;                               // (the buffer was zeroed: a root without a usable child leaves 0)
    }
  }
  __shared__ double part[kCostBlock / 64][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double v = wave_sum(s[k]);
    if (lane == 0) part[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = 0.0;
    for (int w = 0; w < kCostBlock / 64; ++w) v += part[w][threadIdx.x];
    if (v != 0.0) atomicAdd(out + threadIdx.x, v);
  }
}

void launch_gather_tri9(hipStream_t st, const GatherArgs& G) {
  const int64_t lanes = std::max<int64_t>(G.nverts, (int64_t)G.n_prims);
  if (lanes <= 0) return;
  hipLaunchKernelGGL(k_gather_tri9, dim3((unsigned)((lanes + kGatherBlock - 1) / kGatherBlock)), dim3(kGatherBlock), 0, st, G);
}

void launch_tree_cost(hipStream_t st, const float* nodes, int n_nodes, int width, double* sums4) {
  if (n_nodes <= 0) return;
  const dim3 grid((unsigned)((n_nodes + kCostBlock - 1) / kCostBlock)), block(kCostBlock);
  if (width == 4) hipLaunchKernelGGL(k_tree_cost<4>, grid, block, 0, st, nodes, n_nodes, sums4);
  else hipLaunchKernelGGL(k_tree_cost<8>, grid, block, 0, st, nodes, n_nodes, sums4);
}

}  // namespace art
