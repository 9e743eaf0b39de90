// art_display.hip -- the gfx950 kernels of art_auto_exposure_device and art_display_device, whose arithmetic include/art_hip.h states and
// art_display.h defines (the same text tests/display_host compiles with g++).
//
//   k_exposure_histogram   256 lanes per workgroup, a grid-stride walk over the pixels (at most kExpBlocks workgroups, so the number of
//                          global adds is bounded whatever the frame).  A lane reads its pixel's three floats, finds the bin
//                          (dp::exposure_bin: one binary64 log_pos per counted pixel) and adds 1 to the workgroup's counter in LDS
//                          (ds_add_u32, no return value).  After the barrier lane i adds the workgroup's bin i to the state's, if it is
//                          not zero.  Integer adds only, no workgroup waits for another and none is "the last": the words are the same
//                          on every run.  The caller has zeroed the 256 words on the stream.
//   k_exposure_resolve     one wave; lane 0 walks the 254 bins in order (dp::exposure_from_histogram) and writes the state's four words.
//                          A launch of its own after the histogram: stream order is the only synchronisation.
//   k_display              one lane per pixel of the row-major input (dp::display_pixel); the exposure is one uniform load of the
//                          state's first word.  No LDS, no atomics.  With ART_LAYOUT_ADA_XY the stores are strided by the height.
//
// Compulsory bytes per pixel: the histogram reads 12; the display reads 12 and writes 4 (screen), 12 (ldr) or 16 (both).
#include <hip/hip_runtime.h>
#include "art_display.h"
#include "art_kernel_common.h"

namespace art {

constexpr int kExpBlocks = 512;             // 2 workgroups of 256 lanes per CU of an MI355X: every workgroup adds up to 254 words to the state (2048 measured 0.089 ms against 0.054 on a frame over 222 bins, profiles/display/README.md)

__global__ __launch_bounds__(256) void k_exposure_histogram(const ExposureArgs A) {
  __shared__ uint32_t bins[dp::kBins];
  bins[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t n = (uint32_t)A.n, stride = gridDim.x * 256u;         // n <= 2^28 and stride <= 2^19: p + stride cannot wrap
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += stride) atomicAdd(&bins[dp::exposure_bin(A.P, A.color, p)], 1u);
  __syncthreads();
  const uint32_t c = bins[threadIdx.x];
  if (c) atomicAdd(&A.state[4 + threadIdx.x], c);
}

__global__ __launch_bounds__(64) void k_exposure_resolve(const ExposureArgs A) {
  if (threadIdx.x == 0) dp::exposure_from_histogram(A.P, A.state);
}

__global__ __launch_bounds__(256) void k_display(const DisplayArgs A) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= (uint32_t)A.P.W * (uint32_t)A.P.H) return;
  const int y = (int)(p / (uint32_t)A.P.W), x = (int)(p - (uint32_t)y * (uint32_t)A.P.W);
  const float e = A.state ? __builtin_bit_cast(float, A.state[0]) : A.P.exposure;
  dp::display_pixel(A.P, A.color, e, A.screen, A.ldr, x, y);
}

void launch_auto_exposure(hipStream_t st, const ExposureArgs& A) {
  const int blocks = blocks_for(A.n);
  hipLaunchKernelGGL(k_exposure_histogram, dim3((unsigned)(blocks < kExpBlocks ? blocks : kExpBlocks)), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_exposure_resolve, dim3(1), dim3(64), 0, st, A);
}

void launch_display(hipStream_t st, const DisplayArgs& A) {
  hipLaunchKernelGGL(k_display, dim3((unsigned)blocks_for(A.P.W * A.P.H)), dim3(256), 0, st, A);
}

}  // namespace art
