// art_bloom.hip -- the gfx950 kernels of art_bloom_device: the glare pyramid ahead of the display transform, whose arithmetic
// include/art_hip.h states and art_bloom.h defines (the same text tests/bloom_host compiles with g++).
//
//   k_bloom_down<FIRST, KARIS>  one lane per texel of the level being made.  A workgroup of 256 lanes covers a 16 x 16 tile of it (tiles
//                      numbered row-major in a 1-D grid, as art_firefly.hip's); the 36 x 36 texels of the level above that the tile's 13-tap
//                      filters reach are staged in LDS as 16-byte records (20.7 KB), indices clamped while staging, so the filter has no
//                      bounds test and every source texel is fetched once per tile, not up to nine times.  FIRST: the level above is the
//                      frame -- a staged texel is the read rule and the soft knee of a pixel's 12-byte colour, done once per pixel
//                      and tile; the exposure is one uniform load of the state's first word, made only with a prefilter.  KARIS: the five
//                      weighted boxes.  Every lane stages and reaches the barrier; lanes outside the level leave after it.
//   k_bloom_up<MIX>    one lane per texel of the finer level (per pixel of the frame with MIX), 16 x 16 tiles again; the 10 x 10 texels
//                      of the coarser level under the tile are staged (1.6 KB).  Without MIX the lane blends the upsampled texel into
//                      its own D_k in place, which no other lane reads; with MIX it reads its own colour, then writes out3f and
//                      bloom3f, so out3f may be color3f.
//   k_bloom_tail       ONE workgroup of 1024 lanes and up to bl::kTailTexels records (64 KB) of LDS: level P.tail is read from the
//                      pyramid, every level below it is made and blended back up in LDS (bl::tail_down, bl::tail_up: a workgroup
//                      barrier between levels, the lanes striding over a level's texels), and the levels are written back.  It stands
//                      for 2 (M - tail) launches of a few workgroups each.  The words are those of the per-level kernels: the same
//                      functions on the same operands.
// No atomics, no workgroup waits for another, no indexed private array.
//
// Compulsory bytes: 12 per pixel read by the first downsample, 12 read (with out3f) and 12 or 24 written by the mix, and each of the
// pyramid's records (1 / 3 of a record per pixel) written once and read twice (by the level below and by its own blend), then written
// and read once more on the way up.
#include <hip/hip_runtime.h>
#include "art_bloom.h"

namespace art {

constexpr int kBlBlock = 256, kBlTile = 16;
constexpr int kBlDownSide = 2 * kBlTile + 4;      // the staged square of a downsample: columns 2 x0 - 2 .. 2 x0 + 33
constexpr int kBlUpSide = kBlTile / 2 + 2;        // of an upsample: columns (x0 >> 1) - 1 .. (x0 >> 1) + 8

// one launch's two levels: the source is ws x hs, the destination wd x hd in tiles_x columns of tiles
struct BloomLevels { int32_t ws, hs, wd, hd; uint32_t tiles_x; };

template <bool FIRST, bool KARIS>
__global__ __launch_bounds__(kBlBlock) void k_bloom_down(const BloomArgs A, const bl::Rec4* __restrict__ src, bl::Rec4* __restrict__ dst, const BloomLevels G) {
  constexpr int S = kBlDownSide;
  __shared__ bl::Rec4 s_t[S * S];
  const uint32_t ty = blockIdx.x / G.tiles_x, tx = blockIdx.x - ty * G.tiles_x;
  const int x0 = (int)(tx * kBlTile), y0 = (int)(ty * kBlTile);
  for (int i = (int)threadIdx.x; i < S * S; i += kBlBlock) {
    const int cy = i / S, cx = i - cy * S;
    const size_t q = (size_t)bl::clampi(2 * y0 - 2 + cy, G.hs) * (size_t)G.ws + (size_t)bl::clampi(2 * x0 - 2 + cx, G.ws);
    if constexpr (FIRST) s_t[i] = bl::record(bl::level0_pixel(A.P, A.color, q, [&] { return A.state ? __builtin_bit_cast(float, A.state[0]) : A.P.exposure; }));
    else s_t[i] = src[q];
  }
  __syncthreads();
  const int lx = (int)threadIdx.x & (kBlTile - 1), ly = (int)threadIdx.x >> 4;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= G.wd || y >= G.hd) return;              // (after the barrier)
  const int c = 2 * ly * S + 2 * lx;               // t[0][0] of the lane's 6 x 6 texels; all of them lie inside the square
  dst[(size_t)y * (size_t)G.wd + (size_t)x] = bl::record(bl::down13<KARIS>([&](int j, int i) { return bl::texel(s_t[c + i * S + j]); }));
}

template <bool MIX>
__global__ __launch_bounds__(kBlBlock) void k_bloom_up(const BloomArgs A, const bl::Rec4* __restrict__ src, bl::Rec4* __restrict__ dst, const BloomLevels G) {
  constexpr int S = kBlUpSide;
  __shared__ bl::Rec4 s_t[S * S];
  const uint32_t ty = blockIdx.x / G.tiles_x, tx = blockIdx.x - ty * G.tiles_x;
  const int x0 = (int)(tx * kBlTile), y0 = (int)(ty * kBlTile);
  if ((int)threadIdx.x < S * S) {
    const int cy = (int)threadIdx.x / S, cx = (int)threadIdx.x - cy * S;
    s_t[threadIdx.x] = src[(size_t)bl::clampi((y0 >> 1) - 1 + cy, G.hs) * (size_t)G.ws + (size_t)bl::clampi((x0 >> 1) - 1 + cx, G.ws)];
  }
  __syncthreads();
  const int lx = (int)threadIdx.x & (kBlTile - 1), ly = (int)threadIdx.x >> 4;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= G.wd || y >= G.hd) return;              // (after the barrier)
  // the near texel's cell and the far one's: x0 is even, so (x >> 1) - ((x0 >> 1) - 1) = (lx >> 1) + 1; a far index the level clamps is
  // a cell staged from the clamped index
  const int xn = (lx >> 1) + 1, yn = (ly >> 1) + 1, xf = xn + bl::far_step(lx), yf = yn + bl::far_step(ly);
  const bl::T3 u = bl::up2([&](int dx, int dy) { return bl::texel(s_t[(dy ? yf : yn) * S + (dx ? xf : xn)]); });
  const size_t p = (size_t)y * (size_t)G.wd + (size_t)x;
  if constexpr (MIX) bl::mix_pixel(A.P, A.color, p, u, A.out, A.bloom);
  else dst[p] = bl::record(bl::blend(A.P, bl::texel(dst[p]), u));
}

__global__ __launch_bounds__(bl::kTailLanes) void k_bloom_tail(const BloomArgs A) {
  __shared__ bl::Rec4 s_l[bl::kTailTexels];
  bl::Rec4* g = A.pyr + A.P.off[A.P.tail];
  const int first = A.P.w[A.P.tail] * A.P.h[A.P.tail], all = (int)(A.P.off[A.P.made + 1] - A.P.off[A.P.tail]);      // all <= kTailTexels (params_from_abi)
  for (int i = (int)threadIdx.x; i < first; i += bl::kTailLanes) s_l[i] = g[i];
  bl::tail_down(A.P, s_l, (int)threadIdx.x, bl::kTailLanes, [] { __syncthreads(); });
  bl::tail_up(A.P, s_l, (int)threadIdx.x, bl::kTailLanes, [] { __syncthreads(); });
  for (int i = (int)threadIdx.x; i < all; i += bl::kTailLanes) g[i] = s_l[i];
}

void launch_bloom(hipStream_t st, const BloomArgs& A) {
  const bl::Params& P = A.P;
  auto levels = [&](int s, int d) { return BloomLevels{P.w[s], P.h[s], P.w[d], P.h[d], ((uint32_t)P.w[d] + kBlTile - 1) / kBlTile}; };
  auto grid = [&](const BloomLevels& G) { return dim3(G.tiles_x * (((uint32_t)G.hd + kBlTile - 1) / kBlTile)); };      // < 2^31 at 2^28 pixels, as art_firefly.hip's
  BloomLevels G = levels(0, 1);
  const auto first = P.karis ? k_bloom_down<true, true> : k_bloom_down<true, false>;
  hipLaunchKernelGGL(first, grid(G), dim3(kBlBlock), 0, st, A, (const bl::Rec4*)nullptr, A.pyr, G);
  const int last = P.tail ? P.tail : P.made;       // the levels with launches of their own end here
  for (int k = 1; k < last; ++k) {
    G = levels(k, k + 1);
    hipLaunchKernelGGL((k_bloom_down<false, false>), grid(G), dim3(kBlBlock), 0, st, A, (const bl::Rec4*)(A.pyr + P.off[k]), A.pyr + P.off[k + 1], G);
  }
  if (P.tail) hipLaunchKernelGGL(k_bloom_tail, dim3(1), dim3(bl::kTailLanes), 0, st, A);
  for (int k = last - 1; k >= 1; --k) {
    G = levels(k + 1, k);
    hipLaunchKernelGGL((k_bloom_up<false>), grid(G), dim3(kBlBlock), 0, st, A, (const bl::Rec4*)(A.pyr + P.off[k + 1]), A.pyr + P.off[k], G);
  }
  G = levels(1, 0);
  hipLaunchKernelGGL((k_bloom_up<true>), grid(G), dim3(kBlBlock), 0, st, A, (const bl::Rec4*)A.pyr, (bl::Rec4*)nullptr, G);
}

}  // namespace art
