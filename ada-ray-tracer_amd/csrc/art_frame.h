// art_frame.h -- launch interface of art_frame.hip: plain array kernels (resolve, the x-major layouts, padded triangle records, a sum).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace art {

void launch_resolve(hipStream_t st, const float* accum, int n_pixels, float norm_c, uint32_t* screen);
void launch_to_xmajor_f3(hipStream_t st, const float* src, float* dst, int w, int h);
void launch_to_xmajor_u32(hipStream_t st, const uint32_t* src, uint32_t* dst, int w, int h);
void launch_pad_tris(hipStream_t st, const float* src12, float* dst16, int n);
void launch_add_f32(hipStream_t st, const float* src, float* dst, size_t n);

}  // namespace art
