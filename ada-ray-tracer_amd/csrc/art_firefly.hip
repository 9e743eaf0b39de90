// art_firefly.hip -- the gfx950 kernels of art_firefly_device: firefly suppression on a frame ahead of temporal accumulation, whose
// arithmetic include/art_hip.h states and art_firefly.h defines (the same text tests/firefly_host compiles with g++).
//
//   k_firefly_key      one lane per pixel (its linear index, 256 consecutive pixels per workgroup): the pixel's key, l(q) or the quiet NaN,
//                      into the library's key plane.  The window below reads this plane and never the colour, so out3f may be color3f.
//   k_firefly<R, IDS>  one lane per pixel.  A workgroup of 256 lanes covers a 16 x 16 tile of the frame (tiles numbered row-major in a
//                      1-D grid, so no grid dimension can pass its limit at 2^28 pixels).  The tile's keys with their halo, (16 + 2 R)^2
//                      floats (1.6 KB at R = 2), are staged in LDS -- each key is read by up to 25 lanes -- and with IDS the ids beside
//                      them; a position outside the frame is staged as the quiet NaN, which is how a bad pixel reads, so the window has
//                      no bounds test.  Every lane stages and reaches the barrier, lanes outside the frame included; then the lanes
//                      inside keep the four largest keys of their window in four registers by a fixed compare-exchange insertion (no
//                      indexed private array, no scratch memory), read their own colour and moments and write their outputs.  No wave
//                      leaves early: a pixel that is not clamped still has its scaled colour written.  No atomics: every output word
//                      has one owner.
//
// Compulsory bytes per pixel: 12 (colour, key kernel) + 4 (key written) + 4 (key read) + 12 (colour, window kernel) + 12 (out) = 44;
// moments add 16, the id 4, the flag 1.
#include <hip/hip_runtime.h>
#include "art_firefly.h"

namespace art {

constexpr int kFiBlock = 256, kFiTile = 16;

__global__ __launch_bounds__(kFiBlock) void k_firefly_key(const FireflyArgs A) {
  const uint32_t q = blockIdx.x * (uint32_t)kFiBlock + threadIdx.x;            // at most 2^28 pixels (the host's bound)
  if (q >= (uint32_t)A.P.W * (uint32_t)A.P.H) return;
  float r, g, b;
  A.keys[q] = fi::key_of(A.P, A.color, (size_t)q, r, g, b);
}

template <int R, bool IDS>
__global__ __launch_bounds__(kFiBlock) void k_firefly(const FireflyArgs A, const uint32_t tiles_x) {
  constexpr int S = kFiTile + 2 * R;               // the staged square's side
  __shared__ float s_key[S * S];
  __shared__ int32_t s_id[IDS ? S * S : 1];
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = (int)(tx * kFiTile), y0 = (int)(ty * kFiTile);
  for (int i = (int)threadIdx.x; i < S * S; i += kFiBlock) {
    const int cy = i / S, cx = i - cy * S;
    const int qx = x0 - R + cx, qy = y0 - R + cy;
    const bool in = qx >= 0 && qx < A.P.W && qy >= 0 && qy < A.P.H;
    const size_t q = (size_t)(in ? qy : 0) * (size_t)A.P.W + (size_t)(in ? qx : 0);
    s_key[i] = in ? A.keys[q] : fi::qnan();
    if constexpr (IDS) s_id[i] = in ? A.id[q] : 0;
  }
  __syncthreads();
  const int lx = (int)threadIdx.x & (kFiTile - 1), ly = (int)threadIdx.x >> 4;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= A.P.W || y >= A.P.H) return;            // (after the barrier)
  const int c = (ly + R) * S + (lx + R);           // the lane's own cell; its window is c + dy * S + dx, inside the square
  const fi::Top4 t = fi::window<R, IDS>(IDS ? s_id[c] : 0, [&](int dx, int dy) { return s_key[c + dy * S + dx]; },
                                        [&](int dx, int dy) { return s_id[IDS ? c + dy * S + dx : 0]; });
  fi::resolve(A.P, t, A.color, A.moments, (size_t)y * (size_t)A.P.W + (size_t)x, A.out, A.moments_out, A.clamped);
}

void launch_firefly(hipStream_t st, const FireflyArgs& A) {
  const uint32_t n = (uint32_t)A.P.W * (uint32_t)A.P.H;
  hipLaunchKernelGGL(k_firefly_key, dim3((n + kFiBlock - 1) / kFiBlock), dim3(kFiBlock), 0, st, A);
  const uint32_t tiles_x = ((uint32_t)A.P.W + kFiTile - 1) / kFiTile, tiles_y = ((uint32_t)A.P.H + kFiTile - 1) / kFiTile;      // tiles_x * tiles_y <= 2^28 / 256 + W / 16 + H / 16 + 1 < 2^31
  const bool ids = A.id != nullptr;
  const auto k = A.P.radius == 1 ? (ids ? k_firefly<1, true> : k_firefly<1, false>) : (ids ? k_firefly<2, true> : k_firefly<2, false>);
  hipLaunchKernelGGL(k, dim3(tiles_x * tiles_y), dim3(kFiBlock), 0, st, A, tiles_x);
}

}  // namespace art
