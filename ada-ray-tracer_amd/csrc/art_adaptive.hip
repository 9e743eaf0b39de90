// art_adaptive.hip -- the gfx950 kernel of art_adaptive_estimate_device: per pixel the mean colour, the variance of the mean's luminance,
// the relative error and the mask of the next masked pass, whose arithmetic include/art_hip.h states and art_adaptive.h defines (the same
// text tests/adaptive_host compiles with g++).
//
//   k_adaptive_estimate   one lane per pixel; a lane's pixel is its linear index (y * W + x), 256 consecutive pixels of the row-major
//                         frame per workgroup, as in art_temporal.hip.  Every plane is read and written at the lane's own index: a wave
//                         reads 768 contiguous bytes of accum, 512 of moments and 256 of counts, and writes 768 bytes of mean, 256 of
//                         variance, 256 of error and 64 of mask.  No LDS, no atomics, no barrier: every output has one owner.
//
// Compulsory bytes per pixel, every output given: read 12 + 8 + 4 = 24, written 12 + 4 + 4 + 1 = 21.  The arithmetic is one binary32
// reciprocal and a binary64 tail of four divisions and one square root per pixel.  EXPECTATION, not yet measured
// (profiles/adaptive/measure.py is the script): the kernel runs at the rate of its 45 bytes per pixel.
#include <hip/hip_runtime.h>
#include "art_adaptive.h"

namespace art {

constexpr int kAdBlock = 256;

__global__ __launch_bounds__(kAdBlock) void k_adaptive_estimate(const AdaptiveArgs A) {
  const int q = blockIdx.x * kAdBlock + threadIdx.x;             // at most 2^28 pixels (the host's bound)
  if (q >= A.P.n) return;
  const ad::Out o = ad::adaptive_pixel(A.P, A.accum, A.moments, A.counts, (size_t)q);
  if (A.mean) { A.mean[3 * (size_t)q] = o.mean[0]; A.mean[3 * (size_t)q + 1] = o.mean[1]; A.mean[3 * (size_t)q + 2] = o.mean[2]; }
  if (A.variance) A.variance[q] = o.variance;
  if (A.error) A.error[q] = o.error;
  if (A.mask) A.mask[q] = o.mask;
}

void launch_adaptive_estimate(hipStream_t st, const AdaptiveArgs& A) {
  const dim3 grid((unsigned)((A.P.n + kAdBlock - 1) / kAdBlock)), block(kAdBlock);
  hipLaunchKernelGGL(k_adaptive_estimate, grid, block, 0, st, A);
}

}  // namespace art
