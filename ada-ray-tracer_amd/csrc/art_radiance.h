// art_radiance.h -- art_radiance_rays_device (include/art_hip.h): path tracing from the caller's rays.  The two per-item functions of
// art_radiance.hip -- what raygen leaves in bank 0 for a caller's ray, and the walk of a ray's path values into the caller's planes -- as
// host + device text (tests/radiance_host builds them with g++), and the launch interface of that translation unit.
//
// The integrator is the render pass's (art_render.cpp render_batch_records): bank 0 of a batch runs with DevPaths::synth0 = 0 and
// cam_dedup = 0, so bounce 0 is the non-camera instantiation of k_shade_compact and reads, for item w of bank 0, every hot word of
// art_scene.h HotField: the six ray words, HF_HIT (make_record's starting bound, then the trace kernel's hit), HF_SHT and HF_SHMIN (loaded
// with the other words although no shadow test is owed at bounce 0), HF_PDF, HF_FLAGS and HF_SLOT.  raygen_ray_slot writes all of them.
#pragma once
#include "art_shade.h"

namespace art {

// What a batch of the radiance call adds to DevPaths: the caller's arrays, already advanced to the batch's first ray.  A batch holds
// samples [s0, s0 + sn) of rays [r0, r0 + Q.npix); slot = local sample * Q.npix + local ray, Q.pixmap = the rays' RNG keys.
struct RayBatch {
  const float* origins3f; const float* dirs3f;      // 3 floats per ray, 12-byte stride
  float* radiance3f; float* moments2f;              // read-modify-write; moments2f may be nullptr
};

// Slot `slot` of raygen's bank starts as a camera sample does (integrators.adb:37-58 hands PathTrace the ray with StartSample's record:
// previous pdf 1, previous bounce specular) along the ray (o, d), unbounded.  The direction is used as given.
ART_HD void raygen_ray_slot(const DevScene& s, const DevPaths& q, int slot, f3 o, f3 d, const StageCtx& cx = StageCtx()) {
  put_s(hotf<float>(q, HF_OX), slot, o.x); put_s(hotf<float>(q, HF_OY), slot, o.y); put_s(hotf<float>(q, HF_OZ), slot, o.z);
  put_s(hotf<float>(q, HF_DX), slot, d.x); put_s(hotf<float>(q, HF_DY), slot, d.y); put_s(hotf<float>(q, HF_DZ), slot, d.z);
  put_s(hotf<float>(q, HF_PDF), slot, 1.0f);                                   // StartSample (materials.ads:25)
  put_s(hotf<uint32_t>(q, HF_FLAGS), slot, FLAG_ALIVE | FLAG_PREV_SPEC);
  put_s(hotf<uint32_t>(q, HF_SLOT), slot, (uint32_t)slot);
  put_s(hotf<float>(q, HF_SHT), slot, -1.0f);                                  // no shadow ray, no hit of one; nothing is owed
  put_s(hotf<float>(q, HF_SHMIN), slot, 0.0f);
  // HF_HIT (the analytic primitives, intersected at birth) and the ray's 64-byte trace record, staged through cx.stage where the kernel gives one
  emit_ray(s, q, (size_t)slot, (size_t)slot, true, o, d, kInfinity, -1.0f, cx, cx.stage_item);
}

// Ray `pl` of the batch: its sn path values rad_*[t * npix + pl], t = 0 .. sn - 1 in that order, into the caller's planes.
//   out = s_t + out per channel;   l = (0.2126f r + 0.7152f g) + 0.0722f b;   S1 = l + S1;   S2 = l * l + S2      (colour_lum: art_bind_moments' formula)
// the operations of accumulate_pixel / accumulate_pixel_moments without anti-aliasing, on planes indexed by the ray itself.
ART_HD void accumulate_ray(const DevPaths& q, int pl, int sn, float* radiance3f, float* moments2f) {
  float* const a = radiance3f + 3 * (size_t)pl;
  f3 acc = mk3(a[0], a[1], a[2]);
  float s1 = 0.0f, s2 = 0.0f;
  if (moments2f) { s1 = moments2f[2 * (size_t)pl]; s2 = moments2f[2 * (size_t)pl + 1]; }
  for (int t = 0; t < sn; ++t) {
    const size_t si = (size_t)t * (size_t)q.npix + (size_t)pl;
    const f3 color = mk3(q.rad_r[si], q.rad_g[si], q.rad_b[si]);
    acc = color + acc;
    const float l = colour_lum(color);
    s1 = l + s1; s2 = l * l + s2;
  }
  a[0] = acc.x; a[1] = acc.y; a[2] = acc.z;
  if (moments2f) { moments2f[2 * (size_t)pl] = s1; moments2f[2 * (size_t)pl + 1] = s2; }
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_H)
// ---- launch interface of art_radiance.hip (for translation units that have <hip/hip_runtime.h>)
// k_raygen_rays over the Q.P slots of raygen's bank (identity layout: Q.slot_id == nullptr, Q.hot != nullptr)
void launch_raygen_rays(hipStream_t st, const DevScene& S, const DevPaths& Q, const RayBatch& R);
// k_accumulate_rays over the Q.npix rays of the batch, sn samples each
void launch_accumulate_rays(hipStream_t st, const DevPaths& Q, int sn, const RayBatch& R);
// keys[i] = i for i < n: the RNG keys of a call without keys1u that is cut into ray chunks
void launch_iota_keys(hipStream_t st, uint32_t* keys, int n);
#endif

}  // namespace art
