// art_upsample.hip -- the gfx950 kernels of art_upsample_device: joint bilateral upsampling of a lo colour plane under hi and lo feature
// buffers, whose arithmetic include/art_hip.h states and art_upsample.h defines (the same text tests/upsample_host compiles with g++).
//
//   k_upsample_pack   one lane per LO pixel (its linear index, 256 consecutive pixels per workgroup): c(q) = scale * colour (/ the floored
//                     lo albedo) with the lo depth, and the lo normal with the bad-in-guides and bad-in-colour bits, as two 16-byte
//                     records (art_upsample.h), so that a tap of k_upsample costs two 16-byte loads and not seven dword loads from
//                     three planes.  The lo id is read from the caller's plane.
//   k_upsample<FOOT, IDS>   one lane per HI pixel over 16 x 16 tiles (a wave is four rows of 16 pixels): 4 or 16 taps, every tap loaded
//                     from global memory -- neighbouring lanes share their lo taps (at a ratio of 2 a tile reads a 9 x 9 or 11 x 11
//                     patch of lo records), so the lo traffic is served by L1 / L2 -- and the hi guides straight from the caller's
//                     planes.  The sums are per lane in tap order.  No LDS, no atomics: every output pixel has one owner.
//
// Compulsory bytes per hi pixel with every guide: 12 (out) + 1 (fallback) + 12 + 12 + 4 + 4 (the hi guides) = 45, and per lo pixel
// 12 + 12 + 12 + 4 (pack reads) + 32 (records written) + 32 (records read) + 4 (id) = 108, i.e. 27 per hi pixel at a ratio of 2.
#define ART_F64_CONST_FREE      // m1::exp_small's coefficients as plain literals: no asm pin in these kernels (the value is the literal's either way)
#include <hip/hip_runtime.h>
#include "art_upsample.h"

namespace art {

constexpr int kUsBlock = 256, kUsTile = 16;

__global__ __launch_bounds__(kUsBlock) void k_upsample_pack(const UpsampleArgs A) {
  const uint32_t q = blockIdx.x * (uint32_t)kUsBlock + threadIdx.x;            // at most 2^28 lo pixels (the host's bound)
  if (q >= (uint32_t)A.P.LW * (uint32_t)A.P.LH) return;
  us::Rec4 c, g;
  us::pack_lo(A.P, A.lo_color, A.lo_albedo, A.lo_normal, A.lo_depth, (size_t)q, c, g);
  A.lo_c[q] = c; A.lo_g[q] = g;
}

template <int FOOT, bool IDS>
__global__ __launch_bounds__(kUsBlock) void k_upsample(const UpsampleArgs A, const uint32_t tiles_x) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = (int)(tx * kUsTile + (threadIdx.x & (kUsTile - 1))), y = (int)(ty * kUsTile + (threadIdx.x / kUsTile));
  if (x >= A.P.W || y >= A.P.H) return;
  float r, g, b; uint8_t fb;
  us::upsample_pixel<FOOT, IDS>(A.P, A.lo_c, A.lo_g, A.lo_id, A.hi, x, y, r, g, b, fb);
  const size_t p = (size_t)y * (size_t)A.P.W + (size_t)x;
  A.out[3 * p] = r; A.out[3 * p + 1] = g; A.out[3 * p + 2] = b;
  if (A.fallback) A.fallback[p] = fb;
}

void launch_upsample(hipStream_t st, const UpsampleArgs& A) {
  const uint32_t nl = (uint32_t)A.P.LW * (uint32_t)A.P.LH;
  hipLaunchKernelGGL(k_upsample_pack, dim3((nl + kUsBlock - 1) / kUsBlock), dim3(kUsBlock), 0, st, A);
  const uint32_t tiles_x = ((uint32_t)A.P.W + kUsTile - 1) / kUsTile, tiles_y = ((uint32_t)A.P.H + kUsTile - 1) / kUsTile;      // tiles_x * tiles_y <= 2^28 / 256 + W / 16 + H / 16 + 1 < 2^31
  const bool ids = A.P.has_id != 0;
  const auto k = A.P.footprint == 2 ? (ids ? k_upsample<2, true> : k_upsample<2, false>) : (ids ? k_upsample<4, true> : k_upsample<4, false>);
  hipLaunchKernelGGL(k, dim3(tiles_x * tiles_y), dim3(kUsBlock), 0, st, A, tiles_x);
}

}  // namespace art
