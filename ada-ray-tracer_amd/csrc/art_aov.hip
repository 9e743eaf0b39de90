// art_aov.hip -- gfx950 kernels of the first-hit feature buffers (art_render_aovs_device): albedo, shading normal, depth, coverage and
// the primitive / material ids of every pixel's camera rays.
//
//   k_aov_raygen    one lane per (sub-sample, pixel of the slice): camera_dir()'s ray from cam_pos, unbounded, into the SoA slots
//                   k_analytic and the trace kernels read, at slot s * n + local pixel -- the samples-first shape of a render batch, so
//                   that the resolve's loads are dense.  Every ray is live (tfar = Float'Last > 0): none needs k_query_pack's dead-ray
//                   record, the trace launch writes every hit slot.
//   k_aov_resolve   one lane per pixel of the slice: its k DevHits at stride n -> surface_at() and one material fetch per hit -> the
//                   sums (((v0 + v1) + v2) + v3) * 0.25f (k = 1: v0).  The float3 planes are staged through LDS at a stride of 3
//                   dwords (odd: no bank conflict), as k_query_finalize stages its records, so that every store of a wave is 256
//                   contiguous bytes; the scalar planes are stored directly.  A plane that is not wanted costs no store, and the work
//                   that only it needs -- surface_at(), the material fetch -- is not done.  The motion plane of
//                   art_render_aovs_motion_device is a template flag: a third float3 staged the same way, its per-hit arithmetic in
//                   art_motion.h.
//
// Between the two the rays go through the render loop's own trace launch (art_render.cpp trace()).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "art_query.h"
#include "art_motion.h"
#include "art_shade.h"

namespace art {

constexpr int kAovBlock = 256;

__global__ __launch_bounds__(kAovBlock) void k_aov_raygen(const DevFrame F, const DevScene S, const AovArgs A) {
  const int i = blockIdx.x * kAovBlock + threadIdx.x;           // slot: at most 2^28 of them (the host's slice bound)
  if (i >= A.k * A.n) return;
  const int s = i / A.n, l = i - s * A.n;
  const f3 d = camera_dir(F, S, A.pixel0 + (uint32_t)l, (uint32_t)s);
  A.ox[i] = S.cam_pos[0]; A.oy[i] = S.cam_pos[1]; A.oz[i] = S.cam_pos[2];
  A.dx[i] = d.x; A.dy[i] = d.y; A.dz[i] = d.z;
  A.tf[i] = kInfinity;
}

// the motion plane's staging area, a lane's float3 at a stride of 3 dwords like the two below: only the MOTION instantiations call this,
// so only they carry the 3 KB
__device__ __forceinline__ float* motion_lds() { __shared__ float s_mot[3 * kAovBlock]; return s_mot; }

// K: rays per pixel (4 or 1).  MOTION: the call wants the motion plane (AovMotionArgs; art_motion.h) -- its loads (the index triple and
// six vertices of a flat mesh hit, two instance records and the ray of an instanced one) exist in these instantiations only, and the
// others are the kernels they were before the plane existed.  All lanes of the workgroup reach the barrier.
template <int K, bool MOTION>
__global__ __launch_bounds__(kAovBlock) void k_aov_resolve(const DevFrame F, const DevScene S, const std::conditional_t<MOTION, AovMotionArgs, AovArgs> A) {
  __shared__ float s_alb[3 * kAovBlock], s_nrm[3 * kAovBlock];  // a lane's float3 at a stride of 3 dwords
  const int b0 = blockIdx.x * kAovBlock;
  const int l = b0 + (int)threadIdx.x;
  const bool want_surface = A.albedo != nullptr || A.normal != nullptr;      // every ray's surface | ray 0's, for the material id alone
  if (l < A.n) {
    const f3 o = ld3(S.cam_pos), zero = mk3(0.0f, 0.0f, 0.0f), bg = ld3(F.background);
    f3 alb[K], nrm[K]; float dep[K], cov[K];
    [[maybe_unused]] float mx[K], my[K], mz[K];
    int32_t pt = -1, pi = -1, pm = -1;
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const int i = s * A.n + l;
      const DevHit h = A.hit[i];
      const bool hit = h.key != KEY_MISS;
      alb[s] = bg; nrm[s] = zero; dep[s] = hit ? h.t : 0.0f; cov[s] = hit ? 1.0f : 0.0f;
      if (hit && (want_surface || (s == 0 && A.mat != nullptr))) {
        const uint32_t cls = h.key & ~KEY_INDEX_MASK;
        const f3 d = (cls == KEY_SPHERE) ? mk3(A.dx[i], A.dy[i], A.dz[i]) : zero;      // only a sphere's normal needs the hit point
        const Surface sf = surface_at(S, o, d, h.t, h.key, h.u, h.v);
        nrm[s] = sf.normal;
        if (A.albedo) alb[s] = (sf.mat >= 0 && sf.mat < S.n_materials) ? material_albedo(S.materials[sf.mat]) : zero;
        if (s == 0) pm = sf.mat;
      }
      if (s == 0 && hit) {
        const uint32_t cls = h.key & ~KEY_INDEX_MASK;
        pt = (cls == KEY_CORNELL) ? 0 : (cls == KEY_SPHERE) ? 1 : (cls == KEY_QUAD) ? 3 : 2;
        pi = (int32_t)(h.key & KEY_INDEX_MASK);
      }
      if constexpr (MOTION) {
        mo::V3 dl = {0.0f, 0.0f, 0.0f};
        if (hit && (h.key & ~KEY_INDEX_MASK) == KEY_TRI) {
          const bool ray = A.src.inst != nullptr && A.src.prev_m != nullptr;             // only an instanced hit needs the hit point
          dl = mo::hit_delta(A.src, S.cam_pos, h.key, h.t, h.u, h.v, ray ? A.dx[i] : 0.0f, ray ? A.dy[i] : 0.0f, ray ? A.dz[i] : 0.0f);
        }
        mx[s] = dl.x; my[s] = dl.y; mz[s] = dl.z;
      }
    }
    auto mean = [](const float (&v)[K]) { if constexpr (K == 4) return (((v[0] + v[1]) + v[2]) + v[3]) * 0.25f; else return v[0]; };
    if (A.albedo) {
      float x[K], y[K], z[K];
#pragma unroll
      for (int s = 0; s < K; ++s) { x[s] = alb[s].x; y[s] = alb[s].y; z[s] = alb[s].z; }
      s_alb[3 * threadIdx.x] = mean(x); s_alb[3 * threadIdx.x + 1] = mean(y); s_alb[3 * threadIdx.x + 2] = mean(z);
    }
    if (A.normal) {
      float x[K], y[K], z[K];
#pragma unroll
      for (int s = 0; s < K; ++s) { x[s] = nrm[s].x; y[s] = nrm[s].y; z[s] = nrm[s].z; }
      s_nrm[3 * threadIdx.x] = mean(x); s_nrm[3 * threadIdx.x + 1] = mean(y); s_nrm[3 * threadIdx.x + 2] = mean(z);
    }
    if constexpr (MOTION) {
      float* s_mot = motion_lds();
      s_mot[3 * threadIdx.x] = mean(mx); s_mot[3 * threadIdx.x + 1] = mean(my); s_mot[3 * threadIdx.x + 2] = mean(mz);
    }
    if (A.depth) A.depth[l] = mean(dep);
    if (A.alpha) A.alpha[l] = mean(cov);
    if (A.prim_type) A.prim_type[l] = pt;
    if (A.prim_index) A.prim_index[l] = pi;
    if (A.mat) A.mat[l] = pm;
  }
  if constexpr (!MOTION) { if (!want_surface) return; }         // (uniform over the launch)
  __syncthreads();
  const int nw = 3 * (A.n - b0);                                 // floats of this workgroup's pixels that exist
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int k = j * kAovBlock + (int)threadIdx.x;
    if (k < nw) {
      if (A.albedo) A.albedo[3 * (size_t)b0 + k] = s_alb[k];
      if (A.normal) A.normal[3 * (size_t)b0 + k] = s_nrm[k];
      if constexpr (MOTION) A.motion[3 * (size_t)b0 + k] = motion_lds()[k];
    }
  }
}

static inline unsigned aov_blocks(int64_t n) { return (unsigned)((n + kAovBlock - 1) / kAovBlock); }

void launch_aov_raygen(hipStream_t st, const DevFrame& F, const DevScene& S, const AovArgs& A) {
  hipLaunchKernelGGL(k_aov_raygen, dim3(aov_blocks((int64_t)A.k * A.n)), dim3(kAovBlock), 0, st, F, S, A);
}
void launch_aov_resolve(hipStream_t st, const DevFrame& F, const DevScene& S, const AovArgs& A) {
  if (A.k == 4) hipLaunchKernelGGL((k_aov_resolve<4, false>), dim3(aov_blocks(A.n)), dim3(kAovBlock), 0, st, F, S, A);
  else hipLaunchKernelGGL((k_aov_resolve<1, false>), dim3(aov_blocks(A.n)), dim3(kAovBlock), 0, st, F, S, A);
}
void launch_aov_resolve_motion(hipStream_t st, const DevFrame& F, const DevScene& S, const AovMotionArgs& A) {
  if (A.k == 4) hipLaunchKernelGGL((k_aov_resolve<4, true>), dim3(aov_blocks(A.n)), dim3(kAovBlock), 0, st, F, S, A);
  else hipLaunchKernelGGL((k_aov_resolve<1, true>), dim3(aov_blocks(A.n)), dim3(kAovBlock), 0, st, F, S, A);
}

}  // namespace art
