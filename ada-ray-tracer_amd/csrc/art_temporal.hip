// art_temporal.hip -- the gfx950 kernel of art_temporal_device: temporal reprojection, validation and accumulation (the temporal half of
// SVGF, Schied et al. 2017), whose arithmetic include/art_hip.h states and art_temporal.h defines (the same text tests/temporal_host
// compiles with g++).
//
//   k_temporal   one lane per pixel of the current frame; a lane's pixel is its linear index (y * W + x), 256 consecutive pixels of a
//                row-major frame per workgroup, as in art_denoise.hip.  The current planes are read at the lane's own index: a wave reads
//                768 contiguous bytes of colour and of normal, 512 of moments, 256 of depth and of id.  The four taps of the bilinear
//                gather are 16-byte records of the previous history (three per tap: global_load_dwordx4); under a smooth motion the taps
//                of neighbouring lanes are neighbouring records, so a wave's taps fall on a few rows of contiguous lines.  The
//                EXPECTATION, not yet measured (profiles/temporal/measure.py is the script), is that every record then comes from HBM
//                once and is shared through L1 / L2 (a 1920 x 1080 history is 100 MB, the size of the Infinity Cache).  A tap
//                of weight zero is not loaded: with cameras at rest one tap per pixel remains.  The new history leaves as three 16-byte
//                stores per lane (a wave: 1 KB contiguous per plane); out3f leaves as three dword stores per lane at a stride of 12
//                bytes (a wave's 768 bytes are contiguous, but k_atrous<*, true> stages the same plane through LDS; the cost of not doing so
//                here is unmeasured).  No LDS, no atomics, no barrier: every output has one owner.
//
// Compulsory bytes per pixel, every plane given: read 12 (colour) + 8 (moments) + 12 (normal) + 4 (depth) + 4 (id) + 48 (each history record
// once) = 88, written 48 (history) + 12 (out3f) + 4 (variance) + 4 (length) = 68: 156 bytes, 323 MB for a 1920 x 1080 frame.  The arithmetic
// is a few hundred binary32 operations per pixel (three sqrtf, about twenty divisions, one binary64 tail), far below that traffic's time.
//
// Block shape: 256 lanes (4 waves).  The kernel holds no LDS, so occupancy is bounded by registers alone, and 256 consecutive pixels keep a
// workgroup's taps inside a handful of history rows.
#include <hip/hip_runtime.h>
#include "art_temporal.h"

namespace art {

constexpr int kTpBlock = 256;

// MOTION: art_temporal_motion_device with a motion plane, read at the lane's own index like the colour (12 more bytes per pixel: 168).
// The instantiation without it is art_temporal_device's kernel.
template <bool MOTION>
__global__ __launch_bounds__(kTpBlock) void k_temporal(const TemporalArgs A) {
  const int p = blockIdx.x * kTpBlock + threadIdx.x;             // at most 2^28 pixels (the host's bound)
  if (p >= A.n) return;
  const int y = p / A.P.cur.W, x = p - y * A.P.cur.W;
  const tp::Out o = tp::temporal_pixel<MOTION>(A.P, A.color, A.moments, A.normal, A.depth, A.id, A.hist_in, x, y, A.motion);
  A.hist_out[p] = o.h0; A.hist_out[(size_t)A.n + p] = o.h1; A.hist_out[2 * (size_t)A.n + p] = o.h2;
  if (A.out) { A.out[3 * (size_t)p] = o.h0.x; A.out[3 * (size_t)p + 1] = o.h0.y; A.out[3 * (size_t)p + 2] = o.h0.z; }
  if (A.variance_out) A.variance_out[p] = o.variance;
  if (A.length_out) A.length_out[p] = o.h0.w;
}

void launch_temporal(hipStream_t st, const TemporalArgs& A) {
  const dim3 grid((unsigned)((A.n + kTpBlock - 1) / kTpBlock)), block(kTpBlock);
  if (A.has_motion) hipLaunchKernelGGL(k_temporal<true>, grid, block, 0, st, A);
  else hipLaunchKernelGGL(k_temporal<false>, grid, block, 0, st, A);
}

}  // namespace art
