// art_refit_node.h -- device only: the one routine that rewrites a node's child boxes from the boxes below it.  k_refit_level
// (art_refit.hip), k_move_repad and k_move_tlas_level (art_move.hip) are this routine with their own source of a child's tight box.
//
// The rules, each written here and nowhere else:
//   - a child's tight box comes from the caller (`child_box`: the leaf's records, or the tight box an earlier launch stored for the
//     inner node below), with a flag: good, or bad -- nothing usable below it (a bad vertex, a bad instance, an empty tight box);
//   - a bad child is written as an EMPTY box: its binary32 planes all lie at +inf, the node's tight union leaves it out, and its
//     quantised planes are lo = 255, hi = 0 (the near plane behind the far plane) with its entry word unchanged, so no ray enters it;
//   - quantise_node never sees a bad child (its scale-doubling loop needs finite input): the child's slot is marked empty around the
//     call and restored after it;
//   - a good child is padded by the builders' rule (pad_child_box, art_bvh.h) with the caller's two numbers;
//   - an empty slot (ref < 0) is left as the builder wrote it.
// The binary32 operations and their order are the builders' (-ffp-contract=off), so an unmoved tree is reproduced bit for bit.  A launch
// reads only what earlier launches wrote: gfx950's per-XCD L2s are not coherent within a launch, so callers run one launch per level.
#pragma once
#include <hip/hip_runtime.h>

#include "art_bvh.h"
#include "art_refit.h"
#include "art_qnode.h"

namespace art {

// the quantised node's entry words: computed from the packet (a flat tree), or kept as stored (an instanced scene: absolute, with markers)
enum class QEntries { kRecompute, kKeep };

__device__ __forceinline__ bool coord_ok(float v) { return fabsf(v) <= kRefitMaxCoord; }      // (false for NaN and +-inf)

// l..h = the box of the corners of `cnt` triangle records from `tr` on; false when a coordinate is not finite or beyond kRefitMaxCoord
__device__ __forceinline__ bool records_box(const float* tr, int32_t cnt, float l[3], float h[3]) {
  bool ok = true;      // (scalars below: l and h are never indexed by a loop variable, which keeps the caller's packet in registers)
  float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
  for (int r = 0; r < cnt && r < kMaxLeafTris; ++r) {
    const float* p = tr + (size_t)kTriFloats * (size_t)r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = p[3 * k], y = p[3 * k + 1], z = p[3 * k + 2];
      ok = ok && coord_ok(x) && coord_ok(y) && coord_ok(z);
      lx = fminf(lx, x); hx = fmaxf(hx, x); ly = fminf(ly, y); hy = fmaxf(hy, y); lz = fminf(lz, z); hz = fmaxf(hz, z);
    }
  }
  l[0] = lx; l[1] = ly; l[2] = lz; h[0] = hx; h[1] = hy; h[2] = hz;
  return ok;
}

// l..h = a stored tight box (6 floats); false when it is empty: nothing good below
__device__ __forceinline__ bool stored_box(const float* b, float l[3], float h[3]) {
  l[0] = b[0]; l[1] = b[1]; l[2] = b[2]; h[0] = b[3]; h[1] = b[4]; h[2] = b[5];
  return l[0] <= h[0];
}

// packet: the node's binary32 packet (8 W floats, rewritten in place).  qdst: its quantised form (W = 4; nullptr: none).  tight_out: where
// the union of the good children's tight boxes goes (6 floats; nullptr: not wanted).  child_box(j, ref, cnt, l, h) -> good.
template <int W, QEntries E, typename ChildBox>
__device__ __forceinline__ void refit_node(float* packet, QNode* qdst, float* tight_out, float pad_rel, float pad_abs, ChildBox child_box) {
  constexpr int NF = 8 * W;
  float4* const np = reinterpret_cast<float4*>(packet);
  float nd[NF];
#pragma unroll
  for (int k = 0; k < NF / 4; ++k) { const float4 v = np[k]; nd[4 * k] = v.x; nd[4 * k + 1] = v.y; nd[4 * k + 2] = v.z; nd[4 * k + 3] = v.w; }
  float tl[3] = {INFINITY, INFINITY, INFINITY}, th[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool bad[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    bad[j] = false;
    const int32_t ref = __float_as_int(nd[4 * j + 3]), cnt = __float_as_int(nd[4 * W + 4 * j + 3]);
    if (ref < 0) continue;
    float l[3], h[3];
    bad[j] = !child_box(j, ref, cnt, l, h);
    if (bad[j]) {
      for (int a = 0; a < 3; ++a) { nd[4 * j + a] = INFINITY; nd[4 * W + 4 * j + a] = INFINITY; }
      continue;
    }
    for (int a = 0; a < 3; ++a) { tl[a] = fminf(tl[a], l[a]); th[a] = fmaxf(th[a], h[a]); }
    float lo[3], hi[3];
    pad_child_box(l, h, pad_rel, pad_abs, lo, hi);
    for (int a = 0; a < 3; ++a) { nd[4 * j + a] = lo[a]; nd[4 * W + 4 * j + a] = hi[a]; }
  }
  if (tight_out) { tight_out[0] = tl[0]; tight_out[1] = tl[1]; tight_out[2] = tl[2]; tight_out[3] = th[0]; tight_out[4] = th[1]; tight_out[5] = th[2]; }
  if constexpr (W == 4) if (qdst) {
      int32_t keep[W];
#pragma unroll
      for (int j = 0; j < W; ++j) { keep[j] = __float_as_int(nd[4 * j + 3]); if (bad[j]) nd[4 * j + 3] = __int_as_float(-1); }
      QNode q;
      quantise_node(nd, q);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        if (bad[j]) {
          nd[4 * j + 3] = __int_as_float(keep[j]);
          q.rec[j].c0 = 0x00ffffffu; q.rec[j].c1 = 0u;
          if (E == QEntries::kRecompute) {
            const int32_t cnt = __float_as_int(nd[4 * W + 4 * j + 3]);
            q.rec[j].entry = cnt ? (kQEntryLeaf | ((uint32_t)keep[j] * (uint32_t)kQTriBytes) | (uint32_t)cnt) : ((uint32_t)keep[j] * (uint32_t)kQNodeBytes);
          }
        }
        if (E == QEntries::kKeep) q.rec[j].entry = qdst->rec[j].entry;
      }
      *qdst = q;
  }
#pragma unroll
  for (int k = 0; k < NF / 4; ++k) np[k] = make_float4(nd[4 * k], nd[4 * k + 1], nd[4 * k + 2], nd[4 * k + 3]);
}

}  // namespace art
