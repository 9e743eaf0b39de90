// art_query.h -- launch interface of art_query.hip (device-resident ray queries) art_aov.hip (first-hit feature buffers) and
// art_aov_rays.hip (feature buffers along the caller's rays, the frame's camera rays).
#pragma once
#include <hip/hip_runtime.h>
#include "art_scene.h"

namespace art {

// device-resident ray queries (art_query.hip): one slice of at most 2^28 rays.  o3 / d3 / tnear / tfar / out / occluded are the
// caller's buffers advanced to the slice, the rest is the library's scratch.
constexpr int kArtHitWords = 11;      // sizeof(ArtHit) / 4
struct QueryArgs {
  int32_t n;
  const float* o3; const float* d3;   // float3 AoS
  const float* tnear; const float* tfar;   // nullptr: 0 / kInfinity (art_trace_rays' bound)
  float *ox, *oy, *oz, *dx, *dy, *dz, *tf;  // SoA slots of the trace launch (tf < 0: a dead ray)
  float* shm;                         // occlusion: the shadow rule's minimum per ray (written 0); nullptr: closest hit
  DevHit* hit;
  uint32_t* out;                      // ArtHit records (11 dwords each)
  uint8_t* occluded;
};
void launch_query_pack(hipStream_t st, const QueryArgs& Q);
void launch_query_finalize(hipStream_t st, const DevScene& S, const QueryArgs& Q);
void launch_query_occluded(hipStream_t st, const QueryArgs& Q);

// first-hit feature buffers (art_aov.hip, art_device_entries.cpp render_aovs): one slice of n whole pixels, k camera rays each, in the queries'
// scratch.  Ray s of local pixel l lies at slot s * n + l (samples first, like a render batch).  The planes are the caller's, advanced
// to the slice's first pixel; nullptr: not wanted.
struct AovArgs {
  int32_t n, k;                       // pixels of the slice | rays per pixel: 4 (anti-aliasing) or 1
  uint32_t pixel0;                    // the slice's first pixel (y * width + x)
  float *ox, *oy, *oz, *dx, *dy, *dz, *tf;  // SoA slots of the trace launch, k * n of each
  DevHit* hit;
  float* albedo; float* normal;       // 3 floats per pixel
  float* depth; float* alpha;
  int32_t* prim_type; int32_t* prim_index; int32_t* mat;
};
void launch_aov_raygen(hipStream_t st, const DevFrame& F, const DevScene& S, const AovArgs& A);
void launch_aov_resolve(hipStream_t st, const DevFrame& F, const DevScene& S, const AovArgs& A);

// feature buffers along the caller's rays (art_aov_rays.hip, art_device_entries.cpp aovs_rays): one slice of n whole groups, k rays each
// (the caller's rays g * k .. g * k + k - 1 of group g), in the queries' scratch.  Ray s of local group g lies at slot s * n + g, as in
// AovArgs.  o3 / d3 / tnear / tfar and the planes are the caller's, advanced to the slice's first ray and group; nullptr: not given, not wanted.
struct AovRaysArgs {
  int32_t n, k;                       // groups of the slice | rays per group: 1..16
  const float* o3; const float* d3;   // float3 AoS
  const float* tnear; const float* tfar;   // nullptr: 0 / kInfinity
  float *ox, *oy, *oz, *dx, *dy, *dz, *tf;  // SoA slots of the trace launch, k * n of each (tf < 0: a dead ray)
  DevHit* hit;
  float background[3];
  float* albedo; float* normal; float* position;   // 3 floats per group
  float* depth; float* alpha;
  int32_t* prim_type; int32_t* prim_index; int32_t* mat;
};
void launch_aov_rays_pack(hipStream_t st, const AovRaysArgs& A);
void launch_aov_rays_resolve(hipStream_t st, const DevScene& S, const AovRaysArgs& A);
// the frame's camera rays (art_camera_rays_device): n = K * width * height rays, ray s of pixel q at q * K + s, K = 4 with F.aa_on, else 1
void launch_camera_rays(hipStream_t st, const DevFrame& F, const DevScene& S, float* o3, float* d3, int64_t n);

}  // namespace art
