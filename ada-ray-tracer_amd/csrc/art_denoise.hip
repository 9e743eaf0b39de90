// art_denoise.hip -- gfx950 kernels of art_denoise_device, art_denoise_svgf_device and art_denoise_svgf_var_device: the edge-avoiding
// a-trous filters whose arithmetic include/art_hip.h states and art_denoise.h defines (the same text the host builds under tests/ compile
// with g++).
//
//   k_denoise_pack<M>   one lane per pixel, one instantiation per dn::Mode: c_0 = scale * colour (/ the floored albedo), the depth, the
//                    normal, the bad-in-guides flag and the depth gradient, as 16-byte records (art_denoise.h), so that a tap of k_atrous
//                    costs two 16-byte loads and not seven dword loads from four planes.  The two Svgf modes add v_0 (binary64, once per
//                    pixel; from the luminance moments, or from a variance plane at one dword per lane) as the image record's fourth
//                    word; the depth, which held that word, moves to a plane of its own, so a tap stays at two 16-byte loads, plus
//                    one dword load when the depth stop is on (a third 16-byte record would have carried 12 unused bytes per tap).
//   k_atrous<VARIANCE, LAST>   one lane per pixel, iteration i: 25 taps from the image the previous launch wrote, every tap loaded from
//                    global memory (neighbouring lanes share them through L1 / L2; a 1920 x 1080 frame's records are 66 MB, inside the
//                    Infinity Cache).  The sums are per lane in tap order.  VARIANCE (both Svgf modes): the 3 x 3 variance prefilter in
//                    front of the taps (nine more pairs of 16-byte loads per centre, at spacing 1 whatever the iteration: neighbouring
//                    lanes' lines) and v carried through the filter.  LAST: fused with the remodulation, and the float3 output is
//                    staged through LDS at a stride of 3 dwords (odd: no bank conflict), as k_aov_resolve stages its planes, so that
//                    every store of a wave is 256 contiguous bytes; variance_out is one dword per lane, contiguous as it is.  No
//                    atomics: every output pixel has one owner.
//
// A lane's pixel is its linear index (y * W + x): 256 consecutive pixels of a row-major frame per workgroup.
#define ART_F64_CONST_FREE      // m1::exp_small's coefficients as plain literals: no asm pin in these kernels (the value is the literal's either way)
#include <hip/hip_runtime.h>
#include "art_denoise.h"

namespace art {

constexpr int kDnBlock = 256;

template <dn::Mode M>
__global__ __launch_bounds__(kDnBlock) void k_denoise_pack(const DenoiseArgs A) {
  const int p = blockIdx.x * kDnBlock + threadIdx.x;            // at most 2^28 pixels (the host's bound)
  if (p >= A.n) return;
  const int y = p / A.P.W, x = p - y * A.P.W;
  dn::Rec4 c, g; dn::Rec2 d; float z;
  dn::prepare_pixel<M>(A.P, A.n_colours, A.color, A.moments, A.albedo, A.normal, A.depth, x, y, c, g, z, d);
  A.image[0][p] = c; A.guide[p] = g; A.grad[p] = d;
  if constexpr (dn::carries_variance(M)) A.z[p] = z;
}

// The float3 outputs of the workgroup's pixels b0 .. min(b0 + 256, n) - 1, each lane's at a stride of 3 dwords through LDS.  Every lane
// of the workgroup calls it (the barrier); a lane that `has` a pixel brings its r, g, b.
__device__ __forceinline__ void store_rgb_staged(bool has, float r, float g, float b, float* out, int b0, int n) {
  __shared__ float s_out[3 * kDnBlock];
  if (has) { s_out[3 * threadIdx.x] = r; s_out[3 * threadIdx.x + 1] = g; s_out[3 * threadIdx.x + 2] = b; }
  __syncthreads();
  const int nw = 3 * (n - b0);                                   // floats of this workgroup's pixels that exist
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int k = j * kDnBlock + (int)threadIdx.x;
    if (k < nw) out[3 * (size_t)b0 + k] = s_out[k];
  }
}

// iteration i reads image[i & 1] and writes image[(i + 1) & 1] (LAST: the caller's planes)
template <bool VARIANCE, bool LAST>
__global__ __launch_bounds__(kDnBlock) void k_atrous(const DenoiseArgs A, const int i) {
  const int b0 = blockIdx.x * kDnBlock;
  const int p = b0 + (int)threadIdx.x;
  float r = 0.0f, g = 0.0f, b = 0.0f;
  if (p < A.n) {
    const int y = p / A.P.W, x = p - y * A.P.W;
    const dn::Rec4 c = dn::atrous_pixel<VARIANCE>(A.P, A.image[i & 1], A.guide, A.z, A.grad, x, y, i);
    if constexpr (LAST) {
      dn::finish_pixel(A.P, A.albedo, (size_t)p, c, r, g, b);
      if constexpr (VARIANCE) { if (A.variance_out) A.variance_out[p] = c.w; }
    } else {
      A.image[(i + 1) & 1][p] = c;
    }
  }
  if constexpr (LAST) store_rgb_staged(p < A.n, r, g, b, A.out, b0, A.n);
}

void launch_denoise(hipStream_t st, dn::Mode mode, const DenoiseArgs& A, int iterations) {
  using dn::Mode;
  const bool v = dn::carries_variance(mode);
  const auto pack = mode == Mode::Plain ? k_denoise_pack<Mode::Plain> : mode == Mode::Svgf ? k_denoise_pack<Mode::Svgf> : k_denoise_pack<Mode::SvgfVar>;
  const auto step = v ? k_atrous<true, false> : k_atrous<false, false>, last = v ? k_atrous<true, true> : k_atrous<false, true>;
  const dim3 grid((unsigned)((A.n + kDnBlock - 1) / kDnBlock)), block(kDnBlock);
  hipLaunchKernelGGL(pack, grid, block, 0, st, A);
  for (int i = 0; i + 1 < iterations; ++i) hipLaunchKernelGGL(step, grid, block, 0, st, A, i);
  hipLaunchKernelGGL(last, grid, block, 0, st, A, iterations - 1);
}

}  // namespace art
