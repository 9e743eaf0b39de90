// device_kat.hip -- TEST-ONLY measuring instrument (never linked into libart_hip.so, never shipped): runs the product's ART_HD functions
// on the GPU, one item per lane, so that tests/test_gpu_device_kat.py can compare what hipcc made of csrc/art_math.h, art_isect.h and
// art_shade.h for gfx950 with what g++ made of the same text (tests/host_sim, hs_kat_run).  Built with the product's own flags
// (../../ada-ray-tracer_amd/flags.mk).  No persistent state, no streams of its own, no LDS: allocate, copy in, one plain kernel on the
// default stream, synchronise, copy out, free.
#include <hip/hip_runtime.h>
#include <string>
#include "kat_ops.h"

static thread_local std::string g_err;

__global__ void __launch_bounds__(256) k_kat(int op, long long n, const float* in, int in_words, float* out, int out_words, const void* params) {
  const long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
  if (i < n) kat::run_item(op, in + i * in_words, out + i * out_words, params);
}

extern "C" const char* dk_last_error() { return g_err.c_str(); }

// in: n * in_floats_per_item words, out: n * out_floats_per_item words, both HOST pointers; the per-item sizes and params_bytes must be
// the op's (kat::op_shape) -- anything else is refused before a byte moves, so the kernel reads and writes inside its buffers.
extern "C" int dk_run(int op, long long n, const float* in, int in_floats_per_item, float* out, int out_floats_per_item,
                      const void* params, int params_bytes) {
  g_err.clear();
  const kat::OpShape sh = kat::op_shape(op);
  if (op < 0 || op >= kat::OP_COUNT || sh.in_words == 0) { g_err = "dk_run: unknown op"; return (int)hipErrorInvalidValue; }
  if (in_floats_per_item != sh.in_words || out_floats_per_item != sh.out_words) { g_err = "dk_run: item sizes are not the op's"; return (int)hipErrorInvalidValue; }
  if (params_bytes < sh.param_bytes || (sh.param_bytes > 0 && params == nullptr)) { g_err = "dk_run: the op's parameter record is missing or short"; return (int)hipErrorInvalidValue; }
  if (n < 0 || n > (1ll << 24) || (n > 0 && (in == nullptr || out == nullptr))) { g_err = "dk_run: bad item count or null array"; return (int)hipErrorInvalidValue; }
  if (n == 0) return 0;
  const size_t in_bytes = (size_t)n * sh.in_words * 4, out_bytes = (size_t)n * sh.out_words * 4;
  float* d_in = nullptr; float* d_out = nullptr; void* d_par = nullptr;
  hipError_t e = hipSuccess;
  auto step = [&](hipError_t r, const char* what) { if (e == hipSuccess && r != hipSuccess) { e = r; g_err = std::string("dk_run: ") + what + ": " + hipGetErrorString(r); } return e == hipSuccess; };
  if (step(hipMalloc((void**)&d_in, in_bytes), "hipMalloc(in)") && step(hipMalloc((void**)&d_out, out_bytes), "hipMalloc(out)") &&
      step(hipMalloc(&d_par, (size_t)(sh.param_bytes > 0 ? sh.param_bytes : 4)), "hipMalloc(params)") &&
      step(hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice), "copy in") && step(hipMemset(d_out, 0, out_bytes), "clear out") &&
      (sh.param_bytes == 0 || step(hipMemcpy(d_par, params, (size_t)sh.param_bytes, hipMemcpyHostToDevice), "copy params"))) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_kat, dim3(blocks), dim3(256), 0, 0, op, n, d_in, sh.in_words, d_out, sh.out_words, d_par);
    if (step(hipGetLastError(), "launch") && step(hipDeviceSynchronize(), "kernel"))
      step(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost), "copy out");
  }
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (d_par) (void)hipFree(d_par);
  return (int)e;
}
