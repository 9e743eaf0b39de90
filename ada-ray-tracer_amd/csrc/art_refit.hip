// art_refit.hip -- gfx950 kernels of art_refit_device: the CLOSEST mesh's vertices move, the uploaded tree keeps its topology and its
// leaf order, and only the boxes are rewritten.
//
//   k_refit_tris    one lane per triangle record (leaf order): the record's primitive id (word 9) names the index triple, the three new
//                   corners are gathered from the caller's positions and written to the 48-byte record and to its 64-byte padded copy
//                   (the one k_trace_coop reads at width 4); with new normals, lane p also rewrites primitive p's shading record (the
//                   material id stays).  Lanes below nverts count the bad vertices (a coordinate not finite or beyond kRefitMaxCoord).
//   k_refit_level   one launch per tree level, deepest first, one lane per node: refit_node (art_refit_node.h, which states the rules of
//                   a node refit: padding, the tight union, empty boxes for bad children, the quantised form) with a leaf child's box
//                   taken as the min / max over its records and an inner child's as the tight box the previous launch wrote for it.
//                   At width 4 the node is quantised again, entry words recomputed.
//
// A box that holds a bad vertex (a coordinate not finite or beyond kRefitMaxCoord) becomes an empty box; art_synchronize reports the count.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "art_bvh.h"
#include "art_refit.h"
#include "art_refit_node.h"

namespace art {

constexpr int kRefitTrisBlock = 256, kRefitLevelBlock = 128;

__global__ __launch_bounds__(kRefitTrisBlock) void k_refit_tris(const RefitArgs R) {
  const int64_t i = (int64_t)blockIdx.x * kRefitTrisBlock + threadIdx.x;
  if (i < R.nverts) {
    const float* p = R.pos3f + 3 * i;
    if (!(coord_ok(p[0]) && coord_ok(p[1]) && coord_ok(p[2]))) { atomicAdd(&R.bad[0], 1ull); atomicAdd(&R.bad[1], 1ull); }
  }
  if (i < R.n_recs) {
    float* r = R.tris + (size_t)kTriFloats * (size_t)i;
    const int32_t prim = __float_as_int(r[9]);
    if ((uint32_t)prim < (uint32_t)R.n_prims) {
      float v[9];
      for (int k = 0; k < 3; ++k) {
        const float* s = R.pos3f + 3 * (int64_t)R.idx[3 * (size_t)prim + k];
        v[3 * k] = s[0]; v[3 * k + 1] = s[1]; v[3 * k + 2] = s[2];
      }
      reinterpret_cast<float4*>(r)[0] = make_float4(v[0], v[1], v[2], v[3]);
      reinterpret_cast<float4*>(r)[1] = make_float4(v[4], v[5], v[6], v[7]);
      r[8] = v[8];
      if (R.qtris) {
        float* q = R.qtris + (size_t)(kQTriBytes / 4) * (size_t)i;
        reinterpret_cast<float4*>(q)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(q)[1] = make_float4(v[4], v[5], v[6], v[7]);
        q[8] = v[8];
      }
    }
  }
  if (R.nrm3f && i < R.n_prims) {
    float* s = R.m_shade + (size_t)kTriShadeFloats * (size_t)i;
    float n[9];
    for (int k = 0; k < 3; ++k) {
      const float* a = R.nrm3f + 3 * (int64_t)R.idx[3 * (size_t)i + k];
      n[3 * k] = a[0]; n[3 * k + 1] = a[1]; n[3 * k + 2] = a[2];
    }
    reinterpret_cast<float4*>(s)[0] = make_float4(n[0], n[1], n[2], n[3]);
    reinterpret_cast<float4*>(s)[1] = make_float4(n[4], n[5], n[6], n[7]);
    s[8] = n[8];                                                          // (word 9, the material id, is left alone)
  }
}

template <int W>
__global__ __launch_bounds__(kRefitLevelBlock) void k_refit_level(const RefitArgs R, const int32_t* __restrict__ level, int n) {
  const int t = blockIdx.x * kRefitLevelBlock + threadIdx.x;
  if (t >= n) return;
  const int node = level[t];
  refit_node<W, QEntries::kRecompute>(R.nodes + (size_t)node * (8 * W), (W == 4 && R.qnodes) ? R.qnodes + node : nullptr, R.tight + 6 * (size_t)node,
                                      R.inflate_rel, R.inflate_abs, [&](int, int32_t ref, int32_t cnt, float l[3], float h[3]) {
    return cnt > 0 ? records_box(R.tris + (size_t)kTriFloats * (size_t)ref, cnt, l, h) : stored_box(R.tight + 6 * (size_t)ref, l, h);
  });
}

// art_set_camera: lane k < 3 writes cam_pos[k], lane 3 + k cam_matrix[k] of the header the trace kernels take by pointer
__global__ __launch_bounds__(64) void k_set_camera(DevScene* d, const CameraWords C) {
  const int t = threadIdx.x;
  if (t < 3) d->cam_pos[t] = C.w[t];
  else if (t < 19) d->cam_matrix[t - 3] = C.w[t];
}
void launch_set_camera(hipStream_t st, DevScene* d_scene, const CameraWords& C) { hipLaunchKernelGGL(k_set_camera, dim3(1), dim3(64), 0, st, d_scene, C); }

void launch_refit_tris(hipStream_t st, const RefitArgs& R) {
  const int64_t lanes = std::max<int64_t>({R.nverts, (int64_t)R.n_recs, R.nrm3f ? (int64_t)R.n_prims : 0});   // (n_recs = 0: art_rebuild_device, the shading records only)
  if (lanes <= 0) return;
  hipLaunchKernelGGL(k_refit_tris, dim3((unsigned)((lanes + kRefitTrisBlock - 1) / kRefitTrisBlock)), dim3(kRefitTrisBlock), 0, st, R);
}

void launch_refit_level(hipStream_t st, const RefitArgs& R, const int32_t* level_nodes, int n) {
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + kRefitLevelBlock - 1) / kRefitLevelBlock)), block(kRefitLevelBlock);
  if (R.width == 4) hipLaunchKernelGGL(k_refit_level<4>, grid, block, 0, st, R, level_nodes, n);
  else hipLaunchKernelGGL(k_refit_level<8>, grid, block, 0, st, R, level_nodes, n);
}

}  // namespace art
