// art_aov_rays.hip -- gfx950 kernels of the feature buffers along the caller's rays (art_aovs_rays_device) and of the frame's camera rays in
// the caller's memory (art_camera_rays_device).
//
//   k_aov_rays_pack      one lane per ray of the slice: the caller's AoS rays (+ tnear / tfar) -> the SoA slots the trace launch reads, with
//                        k_query_pack's tnear shift and dead-ray rule, at slot s * n + local group -- k_aov_raygen's samples-first shape,
//                        so that the resolve's loads are dense.  Read through LDS as k_query_pack reads them.
//   k_aov_rays_resolve   one lane per group of the slice: its k DevHits at stride n -> per ray what k_query_finalize makes of the hit (the
//                        t0 + t' depth, surface_at() from the ray's own shifted origin) and one material fetch -> the left fold
//                        ((v0 + v1) + ...) / (float)k in running sums, k a run-time 1..16: no array, no scratch memory.  The float3 planes
//                        are staged through LDS at a stride of 3 dwords as k_aov_resolve stages them; a plane that is not wanted costs no
//                        store, and surface_at() and the material fetch are not done where only it needs them.
//   k_camera_rays        one lane per camera ray: ray s of pixel q at q * K + s, the origin cam_pos, the direction camera_dir() -- the
//                        function the render passes and k_aov_raygen call -- staged through LDS, every store of a wave contiguous.
//
// Between pack and resolve the rays go through the render loop's own trace launch (art_render.cpp trace()).
#include <hip/hip_runtime.h>
#include "art_query.h"
#include "art_shade.h"

namespace art {

constexpr int kAovRaysBlock = 256;

__global__ __launch_bounds__(kAovRaysBlock) void k_aov_rays_pack(const AovRaysArgs A) {
  __shared__ float s_o[3 * kAovRaysBlock], s_d[3 * kAovRaysBlock];
  const int m = A.k * A.n;                                       // rays of the slice: at most 2^28 (the host's slice bound), or k
  const int64_t b0 = (int64_t)blockIdx.x * kAovRaysBlock;
  const int i = (int)b0 + (int)threadIdx.x;
  const int64_t nf = 3 * (int64_t)m - 3 * b0;                    // floats of this workgroup's rays that exist
  const float* o3 = A.o3 + 3 * b0;
  const float* d3 = A.d3 + 3 * b0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int k = j * kAovRaysBlock + (int)threadIdx.x;
    if (k < nf) { s_o[k] = o3[k]; s_d[k] = d3[k]; }
  }
  __syncthreads();
  if (i >= m) return;
  f3 o = mk3(s_o[3 * threadIdx.x], s_o[3 * threadIdx.x + 1], s_o[3 * threadIdx.x + 2]);
  const f3 d = mk3(s_d[3 * threadIdx.x], s_d[3 * threadIdx.x + 1], s_d[3 * threadIdx.x + 2]);
  float f = A.tfar ? A.tfar[i] : kInfinity;
  if (A.tnear) {                                                 // k_query_pack's shift: separate multiply and add
    const float tn = A.tnear[i];
    const float t0 = (tn > 0.0f) ? tn : 0.0f;
    o = mk3(o.x + t0 * d.x, o.y + t0 * d.y, o.z + t0 * d.z);
    f = f - t0;
  }
  const bool live = f > 0.0f;
  const int g = i / A.k, s = i - g * A.k;
  const int w = s * A.n + g;                                     // ray s of local group g
  A.ox[w] = o.x; A.oy[w] = o.y; A.oz[w] = o.z; A.dx[w] = d.x; A.dy[w] = d.y; A.dz[w] = d.z;
  A.tf[w] = live ? f : -1.0f;                                    // < 0: the trace kernels skip the ray
  if (!live) A.hit[w] = DevHit{f, KEY_MISS, 0.0f, 0.0f};         // k_query_pack's dead-ray record
}

// All lanes of the workgroup reach the barrier.  The per-hit step (surface_at, the albedo, the ids) is k_aov_resolve's, restated: as a
// function both kernels call it changed the generated code of k_aov_resolve's instantiations, which are to stay as they are.
__global__ __launch_bounds__(kAovRaysBlock) void k_aov_rays_resolve(const DevScene S, const AovRaysArgs A) {
  __shared__ float s_alb[3 * kAovRaysBlock], s_nrm[3 * kAovRaysBlock], s_pos[3 * kAovRaysBlock];   // a lane's float3 at a stride of 3 dwords
  const int b0 = blockIdx.x * kAovRaysBlock;
  const int l = b0 + (int)threadIdx.x;
  const bool want_surface = A.albedo != nullptr || A.normal != nullptr;      // every ray's surface | ray 0's, for the material id alone
  const bool want_t = A.depth != nullptr || A.position != nullptr;
  if (l < A.n) {
    const f3 zero = mk3(0.0f, 0.0f, 0.0f), bg = mk3(A.background[0], A.background[1], A.background[2]);
    f3 alb = zero, nrm = zero, pos = zero; float dep = 0.0f, cov = 0.0f;     // the running sums: v0, then sum + v_s
    int32_t pt = -1, pi = -1, pm = -1;
    for (int s = 0; s < A.k; ++s) {
      const int i = s * A.n + l;
      const DevHit h = A.hit[i];
      const bool hit = h.key != KEY_MISS;
      const uint32_t cls = h.key & ~KEY_INDEX_MASK;
      f3 a = bg, n = zero, p = zero; float t = 0.0f;
      if (hit && want_t) {
        t = h.t;
        const int64_t r = (int64_t)l * A.k + s;                  // the ray as the caller numbers it (from the slice's first)
        if (A.tnear) { const float tn = A.tnear[r]; t = ((tn > 0.0f) ? tn : 0.0f) + t; }      // k_query_finalize's t0 + t'
        if (A.position) {                                        // from the caller's origin: the slot holds it shifted by t0 d
          const f3 o = A.tnear ? ld3(A.o3 + 3 * r) : mk3(A.ox[i], A.oy[i], A.oz[i]);
          p = mk3(o.x + t * A.dx[i], o.y + t * A.dy[i], o.z + t * A.dz[i]);
        }
      }
      if (hit && (want_surface || (s == 0 && A.mat != nullptr))) {
        const bool sphere = cls == KEY_SPHERE;                   // only a sphere's normal needs the hit point, from the ray's own origin
        const f3 o = sphere ? mk3(A.ox[i], A.oy[i], A.oz[i]) : zero, d = sphere ? mk3(A.dx[i], A.dy[i], A.dz[i]) : zero;
        const Surface sf = surface_at(S, o, d, h.t, h.key, h.u, h.v);
        n = sf.normal;
        if (A.albedo) a = (sf.mat >= 0 && sf.mat < S.n_materials) ? material_albedo(S.materials[sf.mat]) : zero;
        if (s == 0) pm = sf.mat;
      }
      if (s == 0 && hit) {
        pt = (cls == KEY_CORNELL) ? 0 : (cls == KEY_SPHERE) ? 1 : (cls == KEY_QUAD) ? 3 : 2;
        pi = (int32_t)(h.key & KEY_INDEX_MASK);
      }
      const float c = hit ? 1.0f : 0.0f;
      if (s == 0) { alb = a; nrm = n; pos = p; dep = t; cov = c; }
      else { alb = alb + a; nrm = nrm + n; pos = pos + p; dep = dep + t; cov = cov + c; }
    }
    const float K = (float)A.k;                                  // one correctly rounded division (k = 1: the value itself)
    if (A.albedo) { s_alb[3 * threadIdx.x] = alb.x / K; s_alb[3 * threadIdx.x + 1] = alb.y / K; s_alb[3 * threadIdx.x + 2] = alb.z / K; }
    if (A.normal) { s_nrm[3 * threadIdx.x] = nrm.x / K; s_nrm[3 * threadIdx.x + 1] = nrm.y / K; s_nrm[3 * threadIdx.x + 2] = nrm.z / K; }
    if (A.position) { s_pos[3 * threadIdx.x] = pos.x / K; s_pos[3 * threadIdx.x + 1] = pos.y / K; s_pos[3 * threadIdx.x + 2] = pos.z / K; }
    if (A.depth) A.depth[l] = dep / K;
    if (A.alpha) A.alpha[l] = cov / K;
    if (A.prim_type) A.prim_type[l] = pt;
    if (A.prim_index) A.prim_index[l] = pi;
    if (A.mat) A.mat[l] = pm;
  }
  if (!want_surface && !A.position) return;                      // (uniform over the launch)
  __syncthreads();
  const int nw = 3 * (A.n - b0);                                 // floats of this workgroup's groups that exist
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int k = j * kAovRaysBlock + (int)threadIdx.x;
    if (k < nw) {
      if (A.albedo) A.albedo[3 * (size_t)b0 + k] = s_alb[k];
      if (A.normal) A.normal[3 * (size_t)b0 + k] = s_nrm[k];
      if (A.position) A.position[3 * (size_t)b0 + k] = s_pos[k];
    }
  }
}

// n = K * width * height rays, K = 4 with F.aa_on, else 1 (at most 2^32: art_resize bounds the frame to 2^30 pixels).  3 b0 is a multiple of 3, so float k of
// the workgroup's origins is component k % 3 of cam_pos.
__global__ __launch_bounds__(kAovRaysBlock) void k_camera_rays(const DevFrame F, const DevScene S, float* o3, float* d3, const int64_t n) {
  __shared__ float s_d[3 * kAovRaysBlock];
  const int64_t b0 = (int64_t)blockIdx.x * kAovRaysBlock;
  const int64_t i = b0 + (int64_t)threadIdx.x;
  if (i < n) {
    const uint32_t q = F.aa_on ? (uint32_t)(i >> 2) : (uint32_t)i, s = F.aa_on ? (uint32_t)(i & 3) : 0u;
    const f3 d = camera_dir(F, S, q, s);
    s_d[3 * threadIdx.x] = d.x; s_d[3 * threadIdx.x + 1] = d.y; s_d[3 * threadIdx.x + 2] = d.z;
  }
  __syncthreads();
  const int64_t nf = 3 * (n - b0);                               // floats of this workgroup's rays that exist
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int k = j * kAovRaysBlock + (int)threadIdx.x;
    if (k < nf) { o3[3 * b0 + k] = S.cam_pos[k % 3]; d3[3 * b0 + k] = s_d[k]; }
  }
}

static inline unsigned aov_rays_blocks(int64_t n) { return (unsigned)((n + kAovRaysBlock - 1) / kAovRaysBlock); }

void launch_aov_rays_pack(hipStream_t st, const AovRaysArgs& A) {
  hipLaunchKernelGGL(k_aov_rays_pack, dim3(aov_rays_blocks((int64_t)A.k * A.n)), dim3(kAovRaysBlock), 0, st, A);
}
void launch_aov_rays_resolve(hipStream_t st, const DevScene& S, const AovRaysArgs& A) {
  hipLaunchKernelGGL(k_aov_rays_resolve, dim3(aov_rays_blocks(A.n)), dim3(kAovRaysBlock), 0, st, S, A);
}
void launch_camera_rays(hipStream_t st, const DevFrame& F, const DevScene& S, float* o3, float* d3, int64_t n) {
  hipLaunchKernelGGL(k_camera_rays, dim3(aov_rays_blocks(n)), dim3(kAovRaysBlock), 0, st, F, S, o3, d3, n);
}

}  // namespace art
