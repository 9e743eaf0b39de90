// art_svgf_spatial.hip -- the gfx950 kernel of art_svgf_spatial_variance_device: SVGF's spatial variance estimate for pixels whose
// history is short, whose arithmetic include/art_hip.h states and art_svgf_spatial.h defines (the same text tests/svgf_spatial_host
// compiles with g++).
//
//   k_svgf_spatial   one lane per pixel.  A workgroup of 256 lanes covers a 16 x 16 tile of the frame (tiles numbered row-major in a 1-D
//                    grid, so no grid dimension can pass its limit at 2^28 pixels); a wave is a 16 x 4 strip of it, so the taps of a
//                    wave's 7 x 7 windows fall on 10 rows of 22 records: the 49 taps of 64 lanes share 220 records per plane.
//                    Every lane loads its word of variance_in and its n (the fourth word of its plane-0 record).  A wave in which no
//                    lane has a short history (one ballot, a wave-uniform branch) stores the word and leaves: the steady state costs
//                    the copy plus the n words.  Otherwise the short lanes run art_svgf_spatial.h's window over global memory, three
//                    16-byte loads per counted tap (the n word first: a tap without history costs one dword), and the long lanes wait
//                    masked.  No LDS, no atomics, no barrier: every output has one owner, and a lane reads its own word of
//                    variance_in before it writes variance_out, so the two may be one plane.
//
// Compulsory bytes per pixel: long history 4 read + 4 written, plus n, which lies at a stride of 16 bytes, so whole lines of plane 0
// travel: 16 more.  Short history: each record of the three planes once, 48, plus the same 8.
#include <hip/hip_runtime.h>
#include "art_svgf_spatial.h"

namespace art {

constexpr int kSvTile = 16;                 // 16 x 16 pixels per workgroup, 16 x 4 per wave

__global__ __launch_bounds__(kSvTile * kSvTile) void k_svgf_spatial(const SvgfSpatialArgs A) {
  const int tile = (int)blockIdx.x;                              // at most 2^28 tiles (the host's bound on the pixels)
  const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
  const int x = tx * kSvTile + ((int)threadIdx.x & (kSvTile - 1)), y = ty * kSvTile + ((int)threadIdx.x >> 4);
  const bool inside = x < A.P.W && y < A.P.H;
  const size_t p = (size_t)y * (size_t)A.P.W + (size_t)x;
  float v = 0.0f;
  bool is_short = false;
  if (inside) {
    v = A.variance_in[p];
    is_short = !sv::long_history(A.P, A.hist[p].w, v);
  }
  if (__builtin_amdgcn_ballot_w64(is_short) != 0ull) {           // wave-uniform: a wave of long histories skips the window altogether
    if (is_short) v = sv::pooled_variance(A.P, A.hist, x, y);
  }
  if (inside) A.variance_out[p] = v;
}

void launch_svgf_spatial(hipStream_t st, const SvgfSpatialArgs& A) {
  const int tiles_y = (A.P.H + kSvTile - 1) / kSvTile;
  const dim3 grid((unsigned)(A.tiles_x * tiles_y)), block(kSvTile * kSvTile);
  hipLaunchKernelGGL(k_svgf_spatial, grid, block, 0, st, A);
}

int svgf_spatial_tiles_x(int width) { return (width + kSvTile - 1) / kSvTile; }

}  // namespace art
