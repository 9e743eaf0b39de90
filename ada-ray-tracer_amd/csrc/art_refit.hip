// art_refit.hip -- gfx950 kernels of art_refit_device: the CLOSEST mesh's vertices move, the uploaded tree keeps its topology and its
// leaf order, and only the boxes are rewritten.
//
//   k_refit_tris    one lane per triangle record (leaf order): the record's primitive id (word 9) names the index triple, the three new
//                   corners are gathered from the caller's positions and written to the 48-byte record and to its 64-byte padded copy
//                   (the one k_trace_coop reads at width 4); with new normals, lane p also rewrites primitive p's shading record (the
//                   material id stays).  Lanes below nverts count the bad vertices (a coordinate not finite or beyond kRefitMaxCoord).
//   k_refit_level   one launch per tree level, deepest first, one lane per node: a leaf child's box is the min / max over its records,
//                   an inner child's box the tight box the previous launch wrote for it.  The node's own tight box (the union) goes to
//                   the scratch array for the level above; every child is padded by the builders' rule (pad_child_box, art_bvh.h) and,
//                   at width 4, the node is quantised again (quantise_node).  Levels pass data only across kernel boundaries: gfx950's
//                   per-XCD L2s are not coherent within a launch.
//
// A box that holds a bad vertex is written as an empty box instead -- the node's tight union leaves it out, its binary32 planes all
// lie at +inf and its quantised planes at lo = 255, hi = 0 with the entry word unchanged -- so no ray enters it, and quantise_node
// (whose scale-doubling loop needs finite input) never sees it.  art_synchronize reports the count.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "art_bvh.h"
#include "art_kernels.h"

namespace art {

constexpr int kRefitTrisBlock = 256, kRefitLevelBlock = 128;

__device__ __forceinline__ bool coord_ok(float v) { return fabsf(v) <= kRefitMaxCoord; }      // (false for NaN and +-inf)

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
  constexpr int NF = 8 * W;
  float4* const np = reinterpret_cast<float4*>(R.nodes + (size_t)node * NF);
  float nd[NF];
#pragma unroll
  for (int k = 0; k < NF / 4; ++k) { const float4 v = np[k]; nd[4 * k] = v.x; nd[4 * k + 1] = v.y; nd[4 * k + 2] = v.z; nd[4 * k + 3] = v.w; }
  float tl[3] = {INFINITY, INFINITY, INFINITY}, th[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool bad[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    bad[j] = false;
    const int32_t ref = __float_as_int(nd[4 * j + 3]), cnt = __float_as_int(nd[4 * W + 4 * j + 3]);
    if (ref < 0) continue;                                                // empty slot: left as the builder wrote it
    float l[3], h[3];
    if (cnt > 0) {
      bool ok = true;
      l[0] = l[1] = l[2] = INFINITY; h[0] = h[1] = h[2] = -INFINITY;
      for (int r = 0; r < cnt && r < kMaxLeafTris; ++r) {
        const float* tr = R.tris + (size_t)kTriFloats * (size_t)(ref + r);
        for (int q = 0; q < 9; ++q) {
          const float v = tr[q];
          ok = ok && coord_ok(v);
          l[q % 3] = fminf(l[q % 3], v); h[q % 3] = fmaxf(h[q % 3], v);
        }
      }
      bad[j] = !ok;
    } else {
      const float* b = R.tight + 6 * (size_t)ref;
      l[0] = b[0]; l[1] = b[1]; l[2] = b[2]; h[0] = b[3]; h[1] = b[4]; h[2] = b[5];
      bad[j] = !(l[0] <= h[0]);                                           // an empty tight box: nothing good below
    }
    if (bad[j]) {
      for (int a = 0; a < 3; ++a) { nd[4 * j + a] = INFINITY; nd[4 * W + 4 * j + a] = INFINITY; }
      continue;
    }
    for (int a = 0; a < 3; ++a) { tl[a] = fminf(tl[a], l[a]); th[a] = fmaxf(th[a], h[a]); }
    float lo[3], hi[3];
    pad_child_box(l, h, R.inflate_rel, R.inflate_abs, lo, hi);
    for (int a = 0; a < 3; ++a) { nd[4 * j + a] = lo[a]; nd[4 * W + 4 * j + a] = hi[a]; }
  }
  float* const tb = R.tight + 6 * (size_t)node;
  tb[0] = tl[0]; tb[1] = tl[1]; tb[2] = tl[2]; tb[3] = th[0]; tb[4] = th[1]; tb[5] = th[2];
  if (W == 4 && R.qnodes) {
    int32_t keep[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { keep[j] = __float_as_int(nd[4 * j + 3]); if (bad[j]) nd[4 * j + 3] = __int_as_float(-1); }   // hidden from quantise_node
    QNode q;
    quantise_node(nd, q);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if (!bad[j]) continue;
      const int32_t cnt = __float_as_int(nd[4 * W + 4 * j + 3]);
      nd[4 * j + 3] = __int_as_float(keep[j]);
      q.rec[j].c0 = 0x00ffffffu; q.rec[j].c1 = 0u;                        // lo = 255, hi = 0: the near plane lies behind the far plane
      q.rec[j].entry = cnt ? (kQEntryLeaf | ((uint32_t)keep[j] * (uint32_t)kQTriBytes) | (uint32_t)cnt) : ((uint32_t)keep[j] * (uint32_t)kQNodeBytes);
    }
    R.qnodes[node] = q;
  }
#pragma unroll
  for (int k = 0; k < NF / 4; ++k) np[k] = make_float4(nd[4 * k], nd[4 * k + 1], nd[4 * k + 2], nd[4 * k + 3]);
}

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
