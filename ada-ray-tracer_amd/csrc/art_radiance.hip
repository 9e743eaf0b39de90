// art_radiance.hip -- gfx950 (CDNA4, wave64): the two ends of art_radiance_rays_device (include/art_hip.h), around the render pass's own
// stages (art_stages.hip) and trace launches (art_trace.hip), none of which it changes:
//
//   k_raygen_rays       one lane per slot of raygen's bank: the caller's ray -> the bank's hot words and the ray's trace record
//   k_accumulate_rays   one lane per ray of the batch: its path values, in sample order, into the caller's radiance (and moments) planes
//   k_iota_keys         the RNG keys of a call without keys that is cut into ray chunks
//
// Per-item functions: art_radiance.h.  No atomics, and no workgroup waits for another.
#include <hip/hip_runtime.h>
#include "art_kernel_common.h"
#include "art_radiance.h"

namespace art {

__global__ __launch_bounds__(256) void k_raygen_rays(const DevScene S, const DevPaths Q, const RayBatch R) {
  __shared__ DevSphere s_sph[kAnalyticLdsSpheres];
  __shared__ DevLight s_lgt[kAnalyticLdsLights];
  StageCtx cx;
  if (S.n_spheres <= kAnalyticLdsSpheres && S.n_lights <= kAnalyticLdsLights) {      // the ray's analytic intersection happens here, as in k_raygen
    if ((int)threadIdx.x < S.n_spheres) s_sph[threadIdx.x] = S.spheres[threadIdx.x];
    if ((int)threadIdx.x < S.n_lights) s_lgt[threadIdx.x] = S.lights[threadIdx.x];
    __syncthreads();
    cx.lds_spheres = as_lds(&s_sph[0]); cx.lds_lights = as_lds(&s_lgt[0]);
  }
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // a wave's 64 records are 4 KB of consecutive bytes; staged through LDS so that every store instruction writes one contiguous kilobyte (k_raygen)
  constexpr int kPitch = 64 + 1;
  __shared__ Rec4 s_stage[4][4 * kPitch];
  const bool staged = Q.has_bvh != 0;
  if (staged) { cx.stage = s_stage[wave]; cx.stage_pitch = kPitch; cx.stage_item = lane; }
  cx.hot_layout = true;
  // The wave's rays.  Its slots [first, first + cnt) are consecutive; where they lie in one sample row (slot = sample * npix + ray) their
  // rays are consecutive too: 3 cnt floats of each of the caller's arrays, fetched as contiguous dwords (64 lanes x 4 bytes per load) into
  // LDS and read back 12 bytes per lane (a stride of 3 words: no bank conflict).  A wave that straddles rows -- the last one of a row, or
  // a batch of fewer than 64 rays -- reads its 12-byte-strided rays directly.
  __shared__ float s_ray[4][2][3 * 64];
  const int first = __builtin_amdgcn_readfirstlane(slot - lane);
  const int cnt = max(0, min(64, Q.P - first));
  const int pl0 = first % Q.npix;
  f3 o = mk3(0.0f, 0.0f, 0.0f), d = o;
  if (pl0 + cnt <= Q.npix) {                               // (wave-uniform)
    const float* const go = R.origins3f + 3 * (size_t)pl0; const float* const gd = R.dirs3f + 3 * (size_t)pl0;
    for (int j = lane; j < 3 * cnt; j += 64) { s_ray[wave][0][j] = go[j]; s_ray[wave][1][j] = gd[j]; }
    wave_lds_sync();
    if (lane < cnt) { o = ld3(&s_ray[wave][0][3 * lane]); d = ld3(&s_ray[wave][1][3 * lane]); }
  } else if (slot < Q.P) {
    const size_t pl = (size_t)(slot % Q.npix);
    o = ld3(R.origins3f + 3 * pl); d = ld3(R.dirs3f + 3 * pl);
  }
  if (slot < Q.P) raygen_ray_slot(S, Q, slot, o, d, cx);
  if (staged) {
    wave_lds_sync();
    const int n_pieces = 4 * cnt;
    Rec4* out = Q.rec + 4 * (size_t)first;
    for (int pc = lane; pc < n_pieces; pc += 64) put_s(out, pc, s_stage[wave][(pc & 3) * kPitch + (pc >> 2)]);      // (read once, by the trace kernel: non-temporal)
  }
}

// SoA reads of the rad planes (consecutive lanes, consecutive words); 12 (8) bytes per lane to the caller's AoS planes
__global__ __launch_bounds__(256) void k_accumulate_rays(const DevPaths Q, int sn, const RayBatch R) {
  const int pl = blockIdx.x * blockDim.x + threadIdx.x;
  if (pl < Q.npix) accumulate_ray(Q, pl, sn, R.radiance3f, R.moments2f);
}

__global__ __launch_bounds__(256) void k_iota_keys(uint32_t* keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = (uint32_t)i;
}

void launch_raygen_rays(hipStream_t st, const DevScene& S, const DevPaths& Q, const RayBatch& R) {
  hipLaunchKernelGGL(k_raygen_rays, dim3(blocks_for(Q.P)), dim3(256), 0, st, S, Q, R);
}
void launch_accumulate_rays(hipStream_t st, const DevPaths& Q, int sn, const RayBatch& R) {
  hipLaunchKernelGGL(k_accumulate_rays, dim3(blocks_for(Q.npix)), dim3(256), 0, st, Q, sn, R);
}
void launch_iota_keys(hipStream_t st, uint32_t* keys, int n) {
  hipLaunchKernelGGL(k_iota_keys, dim3(blocks_for(n)), dim3(256), 0, st, keys, n);
}

}  // namespace art
