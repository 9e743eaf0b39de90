// art_query.hip -- gfx950 kernels of the device-resident ray queries (art_trace_rays_device / art_occluded_rays_device).
//
//   k_query_pack       the caller's AoS rays (+ tnear / tfar) -> the SoA slots k_analytic and k_trace_simple read, with the tnear shift
//                      of gcore's run_batch (o + t0 d, tfar - t0); a ray with an empty interval becomes a dead ray whose miss record is
//                      written here (the trace kernels never touch dead rays).
//   k_query_finalize   DevHit (t, key, u, v) -> the 44-byte ArtHit art_trace_rays builds on the host (surface_at for the normal and the
//                      material, the miss record, the t0 + t' correction), staged through LDS so that every store of a wave is 256
//                      contiguous bytes.
//   k_query_occluded   one byte per ray: the hit record holds a hit.
//
// Between pack and finalize the rays go through the render loop's own trace launch (art_render.cpp trace(): k_analytic + k_trace_coop,
// or k_trace_simple); occlusion runs every ray as a shadow ray of that launch (shadow_begin = 0, sh_min = 0), so the early exit of
// the shadow rule applies.
#include <hip/hip_runtime.h>
#include "art_query.h"
#include "art_shade.h"

namespace art {

constexpr int kQueryBlock = 256;

// AoS -> SoA.  The 3 x 256 floats of a workgroup's origins (and directions) are read as dwords at consecutive addresses into LDS and
// picked up at a stride of 3 dwords (odd: no bank conflict).
__global__ __launch_bounds__(kQueryBlock) void k_query_pack(const QueryArgs Q) {
  __shared__ float s_o[3 * kQueryBlock], s_d[3 * kQueryBlock];
  const int64_t b0 = (int64_t)blockIdx.x * kQueryBlock;
  const int i = (int)b0 + (int)threadIdx.x;
  const int64_t nf = 3 * (int64_t)Q.n - 3 * b0;                 // floats of this workgroup's rays that exist
  const float* o3 = Q.o3 + 3 * b0;
  const float* d3 = Q.d3 + 3 * b0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int k = j * kQueryBlock + (int)threadIdx.x;
    if (k < nf) { s_o[k] = o3[k]; s_d[k] = d3[k]; }
  }
  __syncthreads();
  if (i >= Q.n) return;
  f3 o = mk3(s_o[3 * threadIdx.x], s_o[3 * threadIdx.x + 1], s_o[3 * threadIdx.x + 2]);
  const f3 d = mk3(s_d[3 * threadIdx.x], s_d[3 * threadIdx.x + 1], s_d[3 * threadIdx.x + 2]);
  float f = Q.tfar ? Q.tfar[i] : kInfinity;
  if (Q.tnear) {                                                 // gcore_api.cpp run_batch: separate multiply and add (-ffp-contract=off)
    const float tn = Q.tnear[i];
    const float t0 = (tn > 0.0f) ? tn : 0.0f;
    o = mk3(o.x + t0 * d.x, o.y + t0 * d.y, o.z + t0 * d.z);
    f = f - t0;
  }
  const bool live = f > 0.0f;
  Q.ox[i] = o.x; Q.oy[i] = o.y; Q.oz[i] = o.z; Q.dx[i] = d.x; Q.dy[i] = d.y; Q.dz[i] = d.z;
  Q.tf[i] = live ? f : -1.0f;                                    // < 0: the trace kernels skip the ray
  if (!live) Q.hit[i] = DevHit{f, KEY_MISS, 0.0f, 0.0f};         // what a live ray that hits nothing leaves: t = its bound, u = v = 0
  if (Q.shm) Q.shm[i] = 0.0f;                                    // occlusion: every hit is a far hit of the shadow rule
}

// DevHit -> ArtHit (art_device_entries.cpp trace_rays, the host loop after the download, on the device)
__global__ __launch_bounds__(kQueryBlock) void k_query_finalize(const DevScene S, const QueryArgs Q) {
  constexpr int W = kArtHitWords;
  __shared__ uint32_t s_out[W * kQueryBlock];                    // a lane's record at a stride of 11 dwords (odd: no bank conflict)
  const int64_t b0 = (int64_t)blockIdx.x * kQueryBlock;
  const int i = (int)b0 + (int)threadIdx.x;
  if (i < Q.n) {
    const DevHit h = Q.hit[i];
    uint32_t* r = s_out + W * threadIdx.x;
    r[9] = __float_as_uint(h.u); r[10] = __float_as_uint(h.v);
    if (h.key == KEY_MISS) {
      r[0] = __float_as_uint(h.t); r[1] = 0u;
      r[2] = r[3] = r[4] = r[5] = 0xffffffffu;
      r[6] = r[7] = r[8] = 0u;
    } else {
      const f3 o = mk3(Q.ox[i], Q.oy[i], Q.oz[i]), d = mk3(Q.dx[i], Q.dy[i], Q.dz[i]);
      const Surface sf = surface_at(S, o, d, h.t, h.key, h.u, h.v);
      const uint32_t cls = h.key & ~KEY_INDEX_MASK;
      float t = h.t;
      if (Q.tnear) { const float tn = Q.tnear[i]; t = ((tn > 0.0f) ? tn : 0.0f) + t; }
      r[0] = __float_as_uint(t); r[1] = 1u;
      r[2] = (cls == KEY_CORNELL) ? 0u : (cls == KEY_SPHERE) ? 1u : (cls == KEY_QUAD) ? 3u : 2u;
      r[3] = h.key & KEY_INDEX_MASK; r[4] = (uint32_t)sf.mat_id; r[5] = (uint32_t)sf.mat;
      r[6] = __float_as_uint(sf.normal.x); r[7] = __float_as_uint(sf.normal.y); r[8] = __float_as_uint(sf.normal.z);
    }
  }
  __syncthreads();
  const int64_t nw = W * ((int64_t)Q.n - b0);                    // dwords of this workgroup's records that exist
  uint32_t* out = Q.out + W * b0;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const int k = j * kQueryBlock + (int)threadIdx.x;
    if (k < nw) out[k] = s_out[k];
  }
}

__global__ __launch_bounds__(kQueryBlock) void k_query_occluded(const QueryArgs Q) {
  const int i = blockIdx.x * kQueryBlock + threadIdx.x;
  if (i < Q.n) Q.occluded[i] = (Q.hit[i].key != KEY_MISS) ? 1 : 0;
}

static inline unsigned query_blocks(int n) { return (unsigned)((n + kQueryBlock - 1) / kQueryBlock); }

void launch_query_pack(hipStream_t st, const QueryArgs& Q) {
  hipLaunchKernelGGL(k_query_pack, dim3(query_blocks(Q.n)), dim3(kQueryBlock), 0, st, Q);
}
void launch_query_finalize(hipStream_t st, const DevScene& S, const QueryArgs& Q) {
  hipLaunchKernelGGL(k_query_finalize, dim3(query_blocks(Q.n)), dim3(kQueryBlock), 0, st, S, Q);
}
void launch_query_occluded(hipStream_t st, const QueryArgs& Q) {
  hipLaunchKernelGGL(k_query_occluded, dim3(query_blocks(Q.n)), dim3(kQueryBlock), 0, st, Q);
}

}  // namespace art
