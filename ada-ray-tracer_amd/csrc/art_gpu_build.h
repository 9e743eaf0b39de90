// art_gpu_build.h -- what the GPU builders (art_lbvh.hip: LBVH and PLOC; art_sah.hip: binned SAH) share, included by those two files only:
// the scratch of a build, its event pair, the try-macro, the order-preserving float <-> int encoding, the writer of one slot of a wide-node
// packet, and the tail of a build.  The collapses themselves differ (how a child is opened, how nodes are numbered, what counts as a leaf)
// and stay with their builders.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "art_lbvh.h"
#include "art_qnode.h"

namespace art {
namespace {

#define BUILD_TRY(expr)                                                                       \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(_e); return false; } \
  } while (0)

// device memory of one build, released on every return path
struct Scratch {
  std::vector<void*> ptrs;
  ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
  template <typename T> bool get(T** p, size_t count, std::string& err) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) { err = std::string("hipMalloc: ") + hipGetErrorString(e); return false; }
    ptrs.push_back(q); *p = (T*)q; return true;
  }
};

// the events around the whole build, released on every return path
struct BuildEvents {
  hipEvent_t a = nullptr, b = nullptr;
  ~BuildEvents() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  bool start(hipStream_t st, std::string& err) { BUILD_TRY(hipEventCreate(&a)); BUILD_TRY(hipEventCreate(&b)); BUILD_TRY(hipEventRecord(a, st)); return true; }
};

// order-preserving float <-> int (min / max of encodings = min / max of the floats; -0 sorts below +0, which no result depends on)
__host__ __device__ __forceinline__ int enc(float f) { const int i = __builtin_bit_cast(int, f); return i >= 0 ? i : i ^ 0x7fffffff; }
__host__ __device__ __forceinline__ float dec(int i) { return __builtin_bit_cast(float, i >= 0 ? i : i ^ 0x7fffffff); }
constexpr int kEncPosInf = 0x7f800000;            // enc(+inf): identity of a minimum
constexpr int kEncNegInf = (int)0x807fffffu;      // enc(-inf): identity of a maximum

// Slot j of the packet nd of `width` slots, as a collapse leaves it: the child's box lo3 .. hi3 padded (pad_child_box), ref and cnt in
// word 3 of the slot's lo and hi rows; an unused slot is zeroed (the caller passes ref = -1, cnt = 0 for it; its box is not read).
__device__ __forceinline__ void write_wide_slot(float* nd, int width, int j, bool used, const float lo3[3], const float hi3[3], float inflate_rel, float inflate_abs,
                                                int ref, int cnt) {
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (used) pad_child_box(lo3, hi3, inflate_rel, inflate_abs, lo, hi);
  const int hb = 4 * width;
  nd[4 * j + 0] = lo[0]; nd[4 * j + 1] = lo[1]; nd[4 * j + 2] = lo[2]; nd[4 * j + 3] = __int_as_float(ref);
  nd[hb + 4 * j + 0] = hi[0]; nd[hb + 4 * j + 1] = hi[1]; nd[hb + 4 * j + 2] = hi[2]; nd[hb + 4 * j + 3] = __int_as_float(cnt);
}

// The tail of a build, after the last collapse level (out.nodes, out.n_nodes and out.max_stack are final): at width 4 the quantised form
// of every node, then the end event, the wait for it, and the build's time and size.
inline bool finish_gpu_build(const BvhBuildParams& prm, hipStream_t st, const BuildEvents& ev, int n_tris, GpuBvh& out, std::string& err) {
  if (prm.width == 4 && prm.quantise) {
    BUILD_TRY(hipMalloc(&out.qnodes, (size_t)out.n_nodes * kQNodeBytes));
    launch_quantise_nodes(st, out.nodes, out.n_nodes, out.qnodes);
  }
  BUILD_TRY(hipEventRecord(ev.b, st));
  BUILD_TRY(hipEventSynchronize(ev.b));
  float ms = 0.0f;
  BUILD_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
  BUILD_TRY(hipGetLastError());
  out.n_tris = n_tris; out.build_ms = ms;
  return true;
}

}  // namespace
}  // namespace art
