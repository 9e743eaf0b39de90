// art_motion.h -- the per-hit text of the motion plane of art_render_aovs_motion_device (include/art_hip.h states the arithmetic; this
// is its one definition).  ART_HD functions over plain pointers, no HIP types: art_aov.hip compiles them for gfx950 and tests/motion_host
// compiles the same text with g++ (the arrangement of art_denoise.h with tests/denoise_host and of art_temporal.h with
// tests/temporal_host), so the kernel and the host build cannot drift apart.
//
// A delta is the world-space displacement BACK in time of a camera ray's surface point: where the point was one update ago minus where it
// is.  Only a KEY_TRI hit can have one; every other hit class and a miss give (+0, +0, +0).
#pragma once
#include "art_scene.h"

namespace art {
namespace mo {

struct V3 { float x, y, z; };

// What the deltas are made from.  Flat scene: the mesh's index triples and the caller's two vertex arrays (cur and prev both given, or
// both nullptr).  Instanced scene (inst != nullptr): the instance table in force and the caller's previous matrices (nullptr: no motion).
struct Source {
  const int32_t* idx;              // 3 per primitive of the flat mesh
  const float* cur; const float* prev;      // 3 per vertex
  const DevInstance* inst;         // record j < n_inst = instance j: m and minv in force
  const float* prev_m;             // 12 per instance
  int32_t inst_shift;
};

// row k of a 3 x 4 matrix applied to a point
ART_HD float row(const float* m, int k, float px, float py, float pz) { return ((m[4 * k] * px + m[4 * k + 1] * py) + m[4 * k + 2] * pz) + m[4 * k + 3]; }

// flat scene, primitive `prim` hit at barycentrics (u, v): u weights C, v weights B (ArtHit).  Displacements are interpolated, not
// positions, so an unmoved vertex triple gives exactly +0.
ART_HD V3 flat_delta(const int32_t* idx, const float* cur, const float* prev, uint32_t prim, float u, float v) {
  const size_t a = (size_t)idx[3 * (size_t)prim], b = (size_t)idx[3 * (size_t)prim + 1], c = (size_t)idx[3 * (size_t)prim + 2];
  const float w = (1.0f - u) - v;
  float d[3];
  for (int k = 0; k < 3; ++k) {
    const float da = prev[3 * a + k] - cur[3 * a + k], db = prev[3 * b + k] - cur[3 * b + k], dc = prev[3 * c + k] - cur[3 * c + k];
    d[k] = (w * da + v * db) + u * dc;
  }
  return V3{d[0], d[1], d[2]};
}

// instanced scene: the hit point of the ray cam + t * dir taken to the object space of its instance by the inverse in force, then to the
// world by the previous matrix and by the matrix in force.  Equal words in m_prev and m_cur give exactly 0.
ART_HD V3 inst_delta(const float* m_cur, const float* minv_cur, const float* m_prev, const float* cam, float t, float dx, float dy, float dz) {
  const float wx = cam[0] + t * dx, wy = cam[1] + t * dy, wz = cam[2] + t * dz;
  const float ox = row(minv_cur, 0, wx, wy, wz), oy = row(minv_cur, 1, wx, wy, wz), oz = row(minv_cur, 2, wx, wy, wz);
  return V3{row(m_prev, 0, ox, oy, oz) - row(m_cur, 0, ox, oy, oz), row(m_prev, 1, ox, oy, oz) - row(m_cur, 1, ox, oy, oz),
            row(m_prev, 2, ox, oy, oz) - row(m_cur, 2, ox, oy, oz)};
}

// the delta of one camera ray's hit record (key == KEY_MISS: a miss); (dx, dy, dz) is read for an instanced KEY_TRI hit only
ART_HD V3 hit_delta(const Source& S, const float* cam, uint32_t key, float t, float u, float v, float dx, float dy, float dz) {
  const V3 zero = {0.0f, 0.0f, 0.0f};
  if (key == KEY_MISS || (key & ~KEY_INDEX_MASK) != KEY_TRI) return zero;
  const uint32_t index = key & KEY_INDEX_MASK;
  if (S.inst) {
    if (!S.prev_m) return zero;
    const uint32_t j = index >> S.inst_shift;
    return inst_delta(S.inst[j].m, S.inst[j].minv, S.prev_m + 12 * (size_t)j, cam, t, dx, dy, dz);
  }
  if (!S.cur) return zero;
  return flat_delta(S.idx, S.cur, S.prev, index, u, v);
}

// the pixel's value from its K rays' deltas, one component: the AOV association
ART_HD float mean4(float v0, float v1, float v2, float v3) { return (((v0 + v1) + v2) + v3) * 0.25f; }

}  // namespace mo
}  // namespace art

// ---- launch interface (art_aov.hip's resolve with the motion plane); hipcc only: the g++ builds of the tests take the per-pixel text above and nothing else
#if defined(__HIPCC__)
#include "art_query.h"
namespace art {
// art_render_aovs_motion_device: the same slice with the motion plane (3 floats per pixel, advanced to the slice; never nullptr here) and
// what its deltas are made from (art_motion.h).  A type of its own, so that the kernels without the plane keep their arguments.
struct AovMotionArgs : AovArgs {
  float* motion;
  mo::Source src;
};
void launch_aov_resolve_motion(hipStream_t st, const DevFrame& F, const DevScene& S, const AovMotionArgs& A);
}  // namespace art
#endif
