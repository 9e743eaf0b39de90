// art_denoise.hip -- gfx950 kernels of art_denoise_device: the edge-avoiding a-trous filter whose arithmetic include/art_hip.h states and
// art_denoise.h defines (the same text tests/denoise_host compiles with g++).
//
//   k_denoise_pack   one lane per pixel: c_0 = scale * colour (/ the floored albedo), the depth, the normal, the bad-in-guides flag and the
//                    depth gradient, as 16-byte records (art_denoise.h), so that a tap of k_atrous costs two 16-byte loads and not seven
//                    dword loads from four planes.
//   k_atrous<LAST>   one lane per pixel, iteration i: 25 taps from the image the previous launch wrote, every tap loaded from global
//                    memory (neighbouring lanes share them through L1 / L2; a 1920 x 1080 frame's records are 66 MB, inside the Infinity
//                    Cache).  The sums are per lane in tap order.  LAST: fused with the remodulation, and the float3 output is staged
//                    through LDS at a stride of 3 dwords (odd: no bank conflict), as k_aov_resolve stages its planes, so that every
//                    store of a wave is 256 contiguous bytes.  No atomics: every output pixel has one owner.
//
//
// art_denoise_svgf_device, the variance-guided variant (the second half of art_denoise.h), has kernels of its own:
//   k_svgf_pack      k_denoise_pack plus v_0 from the luminance moments (binary64, once per pixel).  Record layout: the image record is
//                    {r, g, b, v} and the guide record {nx, ny, nz, flags} as before; the depth, which held the image record's fourth
//                    word, moves to a plane of its own.  A tap therefore stays at two 16-byte loads, plus one dword load when the depth
//                    stop is on (a third 16-byte record would have carried 12 unused bytes per tap).
//   k_svgf_atrous<LAST>  as k_atrous, with the 3 x 3 variance prefilter in front of the taps (nine more pairs of 16-byte loads per
//                    centre, at spacing 1 whatever the iteration: neighbouring lanes' lines) and v carried through the filter.  LAST
//                    stages the float3 output through LDS as k_atrous<true> does; variance_out is one dword per lane, contiguous as it is.
//
// art_denoise_svgf_var_device runs the same filter kernels behind k_svgf_var_pack, whose v_0 comes from a variance plane (one dword per lane).
//
// A lane's pixel is its linear index (y * W + x): 256 consecutive pixels of a row-major frame per workgroup.
#define ART_F64_CONST_FREE      // m1::exp_small's coefficients as plain literals: no asm pin in these kernels (the value is the literal's either way)
#include <hip/hip_runtime.h>
#include "art_denoise.h"
#include "art_kernels.h"

namespace art {

constexpr int kDnBlock = 256;

__global__ __launch_bounds__(kDnBlock) void k_denoise_pack(const DenoiseArgs A) {
  const int p = blockIdx.x * kDnBlock + threadIdx.x;            // at most 2^28 pixels (the host's bound)
  if (p >= A.n) return;
  const int y = p / A.P.W, x = p - y * A.P.W;
  dn::Rec4 c, g; dn::Rec2 d;
  dn::pack_pixel(A.P, A.color, A.albedo, A.normal, A.depth, x, y, c, g, d);
  A.image[0][p] = c; A.guide[p] = g; A.grad[p] = d;
}

// iteration i reads image[i & 1] and writes image[(i + 1) & 1] (LAST: the caller's plane).  All lanes of the workgroup reach the barrier.
template <bool LAST>
__global__ __launch_bounds__(kDnBlock) void k_atrous(const DenoiseArgs A, const int i) {
  __shared__ float s_out[LAST ? 3 * kDnBlock : 1];              // a lane's float3 at a stride of 3 dwords
  const int b0 = blockIdx.x * kDnBlock;
  const int p = b0 + (int)threadIdx.x;
  if (p < A.n) {
    const int y = p / A.P.W, x = p - y * A.P.W;
    const dn::Rec4 c = dn::atrous_pixel(A.P, A.image[i & 1], A.guide, A.grad, x, y, i);
    if constexpr (LAST) {
      float r, g, b;
      dn::finish_pixel(A.P, A.albedo, (size_t)p, c, r, g, b);
      s_out[3 * threadIdx.x] = r; s_out[3 * threadIdx.x + 1] = g; s_out[3 * threadIdx.x + 2] = b;
    } else {
      A.image[(i + 1) & 1][p] = c;
    }
  }
  if constexpr (LAST) {
    __syncthreads();
    const int nw = 3 * (A.n - b0);                               // floats of this workgroup's pixels that exist
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int k = j * kDnBlock + (int)threadIdx.x;
      if (k < nw) A.out[3 * (size_t)b0 + k] = s_out[k];
    }
  }
}

void launch_denoise(hipStream_t st, const DenoiseArgs& A, int iterations) {
  const dim3 grid((unsigned)((A.n + kDnBlock - 1) / kDnBlock)), block(kDnBlock);
  hipLaunchKernelGGL(k_denoise_pack, grid, block, 0, st, A);
  for (int i = 0; i + 1 < iterations; ++i) hipLaunchKernelGGL(k_atrous<false>, grid, block, 0, st, A, i);
  hipLaunchKernelGGL(k_atrous<true>, grid, block, 0, st, A, iterations - 1);
}

// ---- art_denoise_svgf_device ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDnBlock) void k_svgf_pack(const SvgfArgs A) {
  const int p = blockIdx.x * kDnBlock + threadIdx.x;            // at most 2^28 pixels (the host's bound)
  if (p >= A.n) return;
  const int y = p / A.P.W, x = p - y * A.P.W;
  dn::Rec4 c, g; dn::Rec2 d; float z;
  dn::svgf_pack_pixel(A.P, A.n_colours, A.color, A.moments, A.albedo, A.normal, A.depth, x, y, c, g, z, d);
  A.image[0][p] = c; A.guide[p] = g; A.z[p] = z; A.grad[p] = d;
}

// iteration i reads image[i & 1] and writes image[(i + 1) & 1] (LAST: the caller's planes).  All lanes of the workgroup reach the barrier.
template <bool LAST>
__global__ __launch_bounds__(kDnBlock) void k_svgf_atrous(const SvgfArgs A, const int i) {
  __shared__ float s_out[LAST ? 3 * kDnBlock : 1];              // a lane's float3 at a stride of 3 dwords
  const int b0 = blockIdx.x * kDnBlock;
  const int p = b0 + (int)threadIdx.x;
  if (p < A.n) {
    const int y = p / A.P.W, x = p - y * A.P.W;
    const dn::Rec4 c = dn::svgf_atrous_pixel(A.P, A.image[i & 1], A.guide, A.z, A.grad, x, y, i);
    if constexpr (LAST) {
      float r, g, b;
      dn::finish_pixel(A.P, A.albedo, (size_t)p, c, r, g, b);
      s_out[3 * threadIdx.x] = r; s_out[3 * threadIdx.x + 1] = g; s_out[3 * threadIdx.x + 2] = b;
      if (A.variance_out) A.variance_out[p] = c.w;
    } else {
      A.image[(i + 1) & 1][p] = c;
    }
  }
  if constexpr (LAST) {
    __syncthreads();
    const int nw = 3 * (A.n - b0);                               // floats of this workgroup's pixels that exist
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int k = j * kDnBlock + (int)threadIdx.x;
      if (k < nw) A.out[3 * (size_t)b0 + k] = s_out[k];
    }
  }
}

void launch_denoise_svgf(hipStream_t st, const SvgfArgs& A, int iterations) {
  const dim3 grid((unsigned)((A.n + kDnBlock - 1) / kDnBlock)), block(kDnBlock);
  hipLaunchKernelGGL(k_svgf_pack, grid, block, 0, st, A);
  for (int i = 0; i + 1 < iterations; ++i) hipLaunchKernelGGL(k_svgf_atrous<false>, grid, block, 0, st, A, i);
  hipLaunchKernelGGL(k_svgf_atrous<true>, grid, block, 0, st, A, iterations - 1);
}

// ---- art_denoise_svgf_var_device: k_svgf_pack with v_0 from the caller's variance plane (A.moments names it); the filter launches are
// art_denoise_svgf_device's own kernels
__global__ __launch_bounds__(kDnBlock) void k_svgf_var_pack(const SvgfArgs A) {
  const int p = blockIdx.x * kDnBlock + threadIdx.x;            // at most 2^28 pixels (the host's bound)
  if (p >= A.n) return;
  const int y = p / A.P.W, x = p - y * A.P.W;
  dn::Rec4 c, g; dn::Rec2 d; float z;
  dn::svgf_var_pack_pixel(A.P, A.color, A.moments, A.albedo, A.normal, A.depth, x, y, c, g, z, d);
  A.image[0][p] = c; A.guide[p] = g; A.z[p] = z; A.grad[p] = d;
}

void launch_denoise_svgf_var(hipStream_t st, const SvgfArgs& A, int iterations) {
  const dim3 grid((unsigned)((A.n + kDnBlock - 1) / kDnBlock)), block(kDnBlock);
  hipLaunchKernelGGL(k_svgf_var_pack, grid, block, 0, st, A);
  for (int i = 0; i + 1 < iterations; ++i) hipLaunchKernelGGL(k_svgf_atrous<false>, grid, block, 0, st, A, i);
  hipLaunchKernelGGL(k_svgf_atrous<true>, grid, block, 0, st, A, iterations - 1);
}

}  // namespace art
