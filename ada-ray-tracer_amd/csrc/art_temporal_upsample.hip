// art_temporal_upsample.hip -- the gfx950 kernels of art_temporal_upsample_device: jittered lo frames accumulated into a hi history,
// whose arithmetic include/art_hip.h states and art_temporal_upsample.h defines (the same text tests/temporal_upsample_host compiles with
// g++).
//
//   k_tu_pack        one lane per LO pixel (its linear index, 256 consecutive pixels per workgroup): scale * colour with m1, m2 with the lo
//                    depth, the lo id and the flags, and the lo normal, as three 16-byte records (art_temporal_upsample.h).
//   k_temporal_upsample<MOTION>   one lane per HI pixel over 16 x 16 tiles (a wave is four rows of 16 pixels): the four lo taps of the
//                    splat, every tap loaded from global memory -- neighbouring lanes share their lo taps (at a ratio of 2 a tile reads a
//                    9 x 9 patch of lo records), so the lo traffic is served by L1 / L2 -- then k_temporal's gather of the hi history
//                    (three 16-byte records per tap, a tap of weight zero not loaded: one tap per pixel between cameras at rest), the hi
//                    guides straight from the caller's planes at the lane's own pixel.  The sums are per lane in tap order.  No LDS, no
//                    atomics, no barrier: every output pixel has one owner.
//
// PACKED, not read directly.  A lo tap read from the caller's planes is ten dword loads from five planes, three of them at a 12-byte
// stride (a wave's addresses then straddle lines, and no load is wider than a dword), and two correctly rounded divisions (S1 / n_cur,
// S2 / n_cur) plus five finiteness tests that every one of the (ratio 2: four) hi pixels tapping that lo pixel would repeat.  Packed, a
// tap is two 16-byte loads (three with normals), aligned, the widest a lane can issue, and the divisions run once per lo pixel.  The
// price is 96 bytes per lo pixel of extra traffic (written once, read from cache) -- 24 per hi pixel at a ratio of 2 -- one small launch,
// and the library's scratch (the host waits when it has to grow, as for art_upsample_device).
//
// Stores.  A lane stores its three history records as 16-byte stores: per plane a wave writes four row segments of 16 x 16 = 256
// contiguous bytes (two whole 128-byte lines each; the tile's 16 rows fill them without a partial line when W is a multiple of 16).
// out3f leaves as three dword stores per lane at a stride of 12 bytes (192 contiguous bytes per row segment), variance and length as one
// dword each (64 bytes per segment), the fallback as one byte.
//
// Compulsory bytes per hi pixel, every plane given: read 12 + 4 + 4 (the hi guides) + 48 (each history record once) = 68, written 48
// (history) + 12 (out3f) + 4 + 4 (variance, length) + 1 (fallback) = 69: 137 (149 with the motion plane); per lo pixel 12 + 8 + 12 + 4 +
// 4 (pack reads) + 48 (records written) + 48 (records read) = 136, i.e. 34 per hi pixel at a ratio of 2: 171 bytes per hi pixel, 355 MB
// for 1920 x 1080 from 960 x 540.
#include <hip/hip_runtime.h>
#include "art_temporal_upsample.h"

namespace art {

constexpr int kTuBlock = 256, kTuTile = 16;

__global__ __launch_bounds__(kTuBlock) void k_tu_pack(const TemporalUpsampleArgs A) {
  const uint32_t q = blockIdx.x * (uint32_t)kTuBlock + threadIdx.x;            // at most 2^28 lo pixels (the host's bound)
  const uint32_t nl = (uint32_t)A.P.LW * (uint32_t)A.P.LH;
  if (q >= nl) return;
  tu::Rec4 a, b, c;
  tu::pack_lo(A.P, A.lo_color, A.lo_moments, A.lo_normal, A.lo_depth, A.lo_id, (size_t)q, a, b, c);
  A.lo_a[q] = a; A.lo_b[q] = b;
  if (A.P.T.has_normal) A.lo_c[q] = c;
}

template <bool MOTION>
__global__ __launch_bounds__(kTuBlock) void k_temporal_upsample(const TemporalUpsampleArgs A, const uint32_t tiles_x) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = (int)(tx * kTuTile + (threadIdx.x & (kTuTile - 1))), y = (int)(ty * kTuTile + (threadIdx.x / kTuTile));
  if (x >= A.P.T.cur.W || y >= A.P.T.cur.H) return;
  const tu::Out o = tu::temporal_upsample_pixel<MOTION>(A.P, A.lo_a, A.lo_b, A.lo_c, A.normal, A.depth, A.id, A.motion, A.hist_in, x, y);
  const size_t n = (size_t)A.P.T.cur.W * (size_t)A.P.T.cur.H, p = (size_t)y * (size_t)A.P.T.cur.W + (size_t)x;
  A.hist_out[p] = o.h0; A.hist_out[n + p] = o.h1; A.hist_out[2 * n + p] = o.h2;
  if (A.out) { A.out[3 * p] = o.h0.x; A.out[3 * p + 1] = o.h0.y; A.out[3 * p + 2] = o.h0.z; }
  if (A.variance_out) A.variance_out[p] = o.variance;
  if (A.length_out) A.length_out[p] = o.h0.w;
  if (A.fallback) A.fallback[p] = o.fallback;
}

void launch_temporal_upsample(hipStream_t st, const TemporalUpsampleArgs& A) {
  const uint32_t nl = (uint32_t)A.P.LW * (uint32_t)A.P.LH;
  hipLaunchKernelGGL(k_tu_pack, dim3((nl + kTuBlock - 1) / kTuBlock), dim3(kTuBlock), 0, st, A);
  const uint32_t tiles_x = ((uint32_t)A.P.T.cur.W + kTuTile - 1) / kTuTile, tiles_y = ((uint32_t)A.P.T.cur.H + kTuTile - 1) / kTuTile;      // tiles_x * tiles_y <= 2^28 / 256 + W / 16 + H / 16 + 1 < 2^31
  if (A.motion) hipLaunchKernelGGL(k_temporal_upsample<true>, dim3(tiles_x * tiles_y), dim3(kTuBlock), 0, st, A, tiles_x);
  else hipLaunchKernelGGL(k_temporal_upsample<false>, dim3(tiles_x * tiles_y), dim3(kTuBlock), 0, st, A, tiles_x);
}

}  // namespace art
