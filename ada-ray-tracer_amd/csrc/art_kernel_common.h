// art_kernel_common.h -- what the kernel units of the render backend (art_trace.hip, art_stages.hip, art_frame.hip) share: the
// wave-level and LDS helpers, the sizes of the analytic tables a workgroup keeps in LDS, and the launchers' two small helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace art {

// hip's __ballot() round-trips the predicate through a VGPR (v_cndmask + v_cmp); the builtin keeps it a lane mask
__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS by 32-bit address (the stack pointer is kept as an LDS byte address: no base + offset add per access)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
__device__ __forceinline__ uint2 lds_load(uint32_t addr) { const u32x2 v = *reinterpret_cast<lds_u32x2*>(addr); return make_uint2(v.x, v.y); }
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ void lds_store(uint32_t addr, uint2 v) {       // two dwords from any two registers (ds_write2_b32): no pair to assemble
  asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" :: "v"(addr), "v"(v.x), "v"(v.y) : "memory");
}

// the scene's spheres and lights a workgroup of k_analytic, k_raygen or k_shade_compact fetches into LDS once
constexpr int kAnalyticLdsSpheres = 64, kAnalyticLdsLights = 16;
constexpr int kAnalyticChunk = 4096;   // rays per workgroup of k_analytic: ONE global atomic per chunk for the queue (a single hot word
                                       // serves only ~88 atomics/us on this chip, so per-wave atomics were the bottleneck)

// ---- launchers
static inline int blocks_for(int n) { return (n + 255) / 256; }

// A launcher's run-time choice between the instantiations of a kernel, written once: f(std::true_type or std::false_type), and the
// same for two choices.  The callee reads the constant as decltype(x)::value.
template <class F> static inline void with_flag(bool a, F&& f) { if (a) f(std::true_type{}); else f(std::false_type{}); }
template <class F> static inline void with_flags(bool a, bool b, F&& f) {
  with_flag(a, [&](auto A) { with_flag(b, [&](auto B) { f(A, B); }); });
}

}  // namespace art
