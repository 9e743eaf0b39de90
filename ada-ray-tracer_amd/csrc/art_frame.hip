// art_frame.hip -- gfx950: the plain array kernels around a render, none of which knows about rays or paths: the accum buffer
// resolved to screen pixels, the x-major layouts of the Ada seam, the padded triangle records and the sum of two framebuffers.
#include <hip/hip_runtime.h>
#include "art_frame.h"
#include "art_kernel_common.h"
#include "art_shade.h"      // resolve_pixel

namespace art {

// AccumBuff -> ScreenBufferData (art_shade.h resolve_pixel)
__global__ __launch_bounds__(256) void k_resolve(const float* accum, int n_pixels, float norm_c, uint32_t* screen) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pixels) screen[i] = resolve_pixel(mk3(accum[3 * (size_t)i], accum[3 * (size_t)i + 1], accum[3 * (size_t)i + 2]), norm_c);
}

// layout conversion at the Ada seam: AccumBuff(x,y) / ScreenBufferData(x,y) are x-major (ray_tracer.ads:35,54)
__global__ __launch_bounds__(256) void k_to_xmajor_f3(const float* src_rowmajor, float* dst_xmajor, int w, int h) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  const int x = i / h, y = i - x * h;
  const size_t s = (size_t)y * w + x;
  dst_xmajor[3 * (size_t)i] = src_rowmajor[3 * s]; dst_xmajor[3 * (size_t)i + 1] = src_rowmajor[3 * s + 1]; dst_xmajor[3 * (size_t)i + 2] = src_rowmajor[3 * s + 2];
}
__global__ __launch_bounds__(256) void k_to_xmajor_u32(const uint32_t* src_rowmajor, uint32_t* dst_xmajor, int w, int h) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  const int x = i / h, y = i - x * h;
  dst_xmajor[i] = src_rowmajor[(size_t)y * w + x];
}

// 48-byte triangle records -> 64-byte padded records for the 4-wide trace kernel
__global__ __launch_bounds__(256) void k_pad_tris(const float* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 16) return;
  const int t = i >> 4, k = i & 15;
  dst[i] = (k < kTriFloats) ? src[(size_t)t * kTriFloats + k] : 0.0f;
}

// dst[i] += src[i]: the framebuffer sum between two contexts that live on the same physical GPU (multi-device rehearsal; distinct
// GPUs use the RCCL reduce).  Written as src + dst: adding exact zeros in any order gives the same bits anyway.
__global__ __launch_bounds__(256) void k_add_f32(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i] + dst[i];
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
void launch_resolve(hipStream_t st, const float* accum, int n_pixels, float norm_c, uint32_t* screen) {
  hipLaunchKernelGGL(k_resolve, dim3(blocks_for(n_pixels)), dim3(256), 0, st, accum, n_pixels, norm_c, screen);
}
void launch_to_xmajor_f3(hipStream_t st, const float* src, float* dst, int w, int h) {
  hipLaunchKernelGGL(k_to_xmajor_f3, dim3(blocks_for(w * h)), dim3(256), 0, st, src, dst, w, h);
}
void launch_to_xmajor_u32(hipStream_t st, const uint32_t* src, uint32_t* dst, int w, int h) {
  hipLaunchKernelGGL(k_to_xmajor_u32, dim3(blocks_for(w * h)), dim3(256), 0, st, src, dst, w, h);
}

void launch_pad_tris(hipStream_t st, const float* src, float* dst, int n) {
  hipLaunchKernelGGL(k_pad_tris, dim3((unsigned)(((size_t)n * 16 + 255) / 256)), dim3(256), 0, st, src, dst, n);
}

void launch_add_f32(hipStream_t st, const float* src, float* dst, size_t n) {
  hipLaunchKernelGGL(k_add_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, n);
}

}  // namespace art
