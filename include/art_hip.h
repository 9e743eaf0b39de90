/*
 * art_hip.h -- C ABI of libart_hip.so, the MI355X (gfx950) render backend for FROL256/ada-ray-tracer.
 *
 * Plain C types only (Interfaces.C.int / float / unsigned, System.Address on the Ada side).
 * Two groups of entry points:
 *
 *  1. Frame-level calls (art_*): what Ray_Tracer.Render_Pass (ray_tracer.adb:240-293) forwards to
 *     instead of waking its Path_Trace_Thread tasks -- the per-pixel DoPass loop
 *     (ray_tracer-integrators.adb:25-71), PathTrace x3 (integrators.adb:82-301),
 *     Scene.Find_Closest_Hit (scene.adb:56-86), Compute_Shadow (ray_tracer.adb:100-132), the accum
 *     and the gamma/tonemap/pack resolve (ray_tracer.adb:281-291) all run on the GPU.
 *
 *  2. The legacy geometry-core seam (gcore_*): the six symbols scene_hydra_embree.adb:37-66 imports
 *     and cpp/embree_connect.cpp:51-244 defines on top of Embree 3.7.  Same names and return types;
 *     counts are element counts (the reference passes 'Size in bits, scene_hydra_embree.adb:259-262).
 *
 * Error convention: art_* return 0 on success, non-zero on failure, text via art_last_error();
 * nothing in this library calls exit() (embree_connect.cpp:28-49 does).  gcore_* keep the reference's
 * return types (0 / false on failure).  Rendering and batched queries have NO CPU fallback: without a usable HIP device
 * every call that needs one fails with a message.  One documented host path exists on the legacy seam: a SINGLE-ray
 * gcore_closest_hit is answered on the calling thread by a walk of the committed tree (the product's own walker, the GPU kernels'
 * boxes and triangle arithmetic: gcore_set_single_ray_on_gpu below; SURVEY 8(b) -- a kernel launch per ray is what that call pattern
 * cannot afford).  The tree itself is always built and committed on the GPU box; nothing routes through the test oracle.
 *
 * Threading: art_* are single-caller (Render_Pass is only called from the environment task,
 * test.adb:50); gcore_closest_hit may be called concurrently (it is in the reference, from up to 28
 * tasks) and is serialised internally.
 */
#ifndef ART_HIP_H
#define ART_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- flattened scene description (host pointers, copied during art_upload_scene) ------------- */

/* materials.ads:58-130 flattened: type tag + parameters */
enum { ART_MAT_NULL = 0, ART_MAT_LIGHT = 1, ART_MAT_LAMBERT = 2, ART_MAT_MIRROR = 3, ART_MAT_GLASS = 4, ART_MAT_PHONG = 5 };
typedef struct ArtMaterial {
  int32_t type;
  int32_t light;     /* LIGHT: index into lights (MaterialLight.lref) */
  float   p[8];      /* LAMBERT kd[3] | MIRROR reflection[3] | GLASS reflection[3] transparency[3] ior | PHONG reflection[3] cosPower */
} ArtMaterial;

/* lights.ads:36-55 */
enum { ART_LIGHT_RECT = 0, ART_LIGHT_SPHERE = 1 };
typedef struct ArtLight {
  int32_t shape;
  int32_t mat;       /* material-table index of the MaterialLight referring to this light */
  float boxMin[3], boxMax[3], normal[3];   /* AreaLight   */
  float center[3], radius;                 /* SphereLight */
  float intensity[3];
  float surfaceArea;
} ArtLight;

/* geometry.ads:21-25 */
typedef struct ArtSphere { float pos[3]; float r; int32_t mat; } ArtSphere;

/* geometry.ads:94-101.  mode selects the search semantics:
 *   ART_MESH_REFERENCE_BF : IntersectMeshBF verbatim (geometry.adb:266-323: bbox early-out, index-order
 *                           scan with the (t, t+1e-6) window, matId forced to 2) -- for the reference's own
 *                           8-triangle pyramid; O(N) per ray.
 *   ART_MESH_CLOSEST      : true closest hit through the BVH (the semantics Embree provides at
 *                           gcore_closest_hit), reference Moeller-Trumbore arithmetic, material_ids honoured. */
enum { ART_MESH_REFERENCE_BF = 0, ART_MESH_CLOSEST = 1 };
typedef struct ArtMesh {
  int32_t mode;
  int32_t nverts, ntris;
  const float*   pos;     /* 3*nverts, world space (LoadMeshFromVSGF transforms positions only) */
  const float*   nrm;     /* 3*nverts */
  const float*   uv;      /* 2*nverts, may be NULL (treated as zeros, geometry.adb:565-566) */
  const int32_t* idx;     /* 3*ntris */
  const int32_t* matid;   /* ntris (ignored in REFERENCE_BF mode) */
  float bbmin[3], bbmax[3];   /* used by REFERENCE_BF (geometry.adb:273) */
} ArtMesh;

/* One instance of a mesh (round 5; the reference: gcore_instance_meshes, embree_connect.cpp:147-184 -- RTC_FORMAT_FLOAT3X4_ROW_MAJOR read from
 * the first 12 floats of a 16-float block, :169).  m: object -> world. */
typedef struct ArtInstance { int32_t mesh; float m[12]; } ArtInstance;

typedef struct ArtSceneDesc {
  int32_t n_spheres;   const ArtSphere*   spheres;
  int32_t has_cornell;                              /* scene.ads:75-80 */
  float   cb_min[3], cb_max[3];
  int32_t cb_mat[6];
  float   cb_nrm[6][3];
  int32_t n_lights;    const ArtLight*    lights;   /* the reference has exactly one (scene.adb:45-48) */
  int32_t n_materials; const ArtMaterial* materials;
  int32_t n_meshes;    const ArtMesh*     meshes;   /* at most one per mode -- unless n_instances > 0 */
  float   cam_pos[3];                               /* scene.ads:27-32 */
  float   cam_matrix[16];                           /* row-major float4x4 */
  /* Instanced scenes (n_instances > 0): meshes[] are then object-space prototypes, any number of them, every one ART_MESH_CLOSEST, and
   * the scene's mesh geometry is instances[]: instance i shows mesh instances[i].mesh under its 3x4.  The render loop walks a tree over
   * the instances and one tree per mesh (memory O(meshes + instances)); the picture is that of the FLATTENED scene, bit for bit --
   * corners transformed by m (m[0] x + m[1] y + m[2] z + m[3], evaluated left to right in binary32), vertex normals by the inverse
   * transpose of its 3x3 and normalised, triangles in the order (instance, triangle of the mesh).  Cooperative trace kernel only. */
  int32_t n_instances; const ArtInstance* instances;
} ArtSceneDesc;

/* ---- render control --------------------------------------------------------------------------- */

enum { ART_RT_DEBUG = 0, ART_RT_WHITTED = 1, ART_PT_STUPID = 2, ART_PT_SHADOW = 3, ART_PT_MIS = 4 };  /* ray_tracer.ads:40 */
enum { ART_LAYOUT_ADA_XY = 0,   /* AccumBuff(x,y) / ScreenBufferData(x,y): element (x,y) at x*height + y (ray_tracer.ads:35,54) */
       ART_LAYOUT_ROW_MAJOR = 1 /* element (x,y) at y*width + x (Bitmap.Image.data, test.adb:65) */ };

/* the mutable package variables Render_Pass reads (ray_tracer.ads:20-32), passed per call */
typedef struct ArtPassParams {
  int32_t  render_type;     /* g_rend_type */
  int32_t  aa_on;           /* Anti_Aliasing_On */
  int32_t  max_depth;       /* Max_Trace_Depth, 1..16 */
  int32_t  vthreads;        /* Threads_Num: the pass adds vthreads * (aa_on ? 4 : 1) samples per pixel */
  float    background[3];   /* Background_Color */
  uint64_t seed;            /* keys the counter-based RNG (replaces Float_Random.Reset, ray_tracer.adb:147) */
  int32_t  layout;          /* layout of the host buffers handed to this call */
} ArtPassParams;

typedef struct ArtStats {
  uint64_t rays;            /* closest-hit queries issued (camera + bounce + shadow), cumulative since art_resize */
  uint64_t samples;         /* camera samples, cumulative */
  double   trace_ms;        /* GPU time inside the trace kernel, cumulative (HIP events) */
  double   pass_ms;         /* GPU time of whole passes (all kernels), cumulative */
  uint64_t trace_launches;
  uint64_t box_tests, tri_tests, node_visits, leaf_visits, traced_rays;  /* only filled by art_trace_rays(stats) / option count_tests */
  uint64_t node_phase_iters, leaf_phase_iters, wave_iters;               /* cooperative kernel: wave-level loop counters (count_tests) */
  uint64_t lost_paths;      /* self-check of the compacted work sets: paths that needed an item and had none; must stay 0 */
} ArtStats;

typedef struct ArtHit {          /* geometry.ads:57-67 flattened */
  float   t;
  int32_t is_hit;
  int32_t prim_type;             /* Primitive'Pos: 0 plane, 1 sphere, 2 triangle, 3 quad; -1 miss */
  int32_t prim_index;
  int32_t mat_id;
  int32_t mat;
  float   normal[3];
  float   u, v;                  /* triangle barycentrics (weight of C, weight of B; geometry.adb:245-246) */
} ArtHit;

typedef struct ArtBvhInfo { int32_t n_nodes, n_tris, max_stack, node_width; double build_ms; } ArtBvhInfo;   /* nodes: 8*node_width floats each */

int  art_init(int device_ordinal);                       /* -1: keep the current HIP device */
/* One process, n GPUs of the node (the Ada host calls Render_Pass from one task: ray_tracer.adb:240-293, test.adb:50).  ordinals ==
 * NULL: devices 0..n-1.  Scene and BVH are replicated, device k owns the 32x32 pixel tiles (bx, by) with (bx + skew by) mod n == k
 * (skew = 3, or 5 when 3 divides n, or 7 when 15 divides n: tiles dealt along diagonals, csrc/art_host_scene.cpp build_pixmap -- an
 * integrator that needs the map should not recompute it from this sentence but take the rule from there), and the float3
 * framebuffers are added into device 0 by ONE RCCL reduce over xGMI whenever the image is asked for (art_render_pass with host
 * pointers, art_download, art_reduce).  The image is bit-identical for any n.  Call INSTEAD of art_init; art_set_stream /
 * art_set_shard / art_bind_accum are single-device calls and fail afterwards.  Repeating one ordinal n times rehearses the whole
 * path on a single GPU (the reduce is then a local sum). */
int  art_init_devices(int32_t n, const int32_t* ordinals);
int32_t art_device_count(void);
int  art_reduce(void);                                   /* enqueue the framebuffer reduce now (no-op with one device) */
/* What the multi-device path really did (round 5: a bench line has to show how many ranks RCCL saw, not be taken on trust).
 * Filled after art_synchronize: rccl_ranks = ncclCommCount of the communicator the reduces ran on (0: no communicator -- one device
 * without ART_FORCE_RCCL, or n contexts on one GPU, whose sum is a chain of local adds); reduce_ms = GPU time of the reduces on device
 * 0's stream (HIP events around the grouped ncclReduce / the adds; it INCLUDES the time device 0's stream waits in the collective for
 * the slowest device), cumulative since art_resize; device_pass_ms[k] = GPU time of device k's render passes (HIP events on its stream),
 * cumulative.  Round 6, n > 1 devices only -- the host clock at which every device's stream reached the start and the end of each pass
 * (hipLaunchHostFunc: one clock for all devices): device_busy_ms[k] = end - start, device_idle_ms[k] = the slowest device's end - device
 * k's end (what an uneven tile deal costs), device_start_skew_ms[k] = device k's start - the first device's start (what enqueueing
 * device after device costs), all summed over the passes; passes_overlapped counts the passes in which every device had started before
 * any had finished -- Render_Pass releases all its workers before it waits for one, ray_tracer.adb:271-277. */
typedef struct ArtReduceInfo {
  int32_t devices;               /* contexts of this process (art_init_devices n) */
  int32_t rccl_ranks;            /* ranks of the RCCL communicator, 0 = none */
  int32_t path;                  /* 0 nothing to reduce, 1 grouped ncclReduce, 2 local adds (contexts on one GPU) */
  int32_t reduces;               /* reduces enqueued since art_resize */
  double  reduce_ms;             /* cumulative */
  double  device_pass_ms[8];     /* per device, cumulative */
  double  device_busy_ms[8], device_idle_ms[8], device_start_skew_ms[8];
  int32_t passes, passes_overlapped;
} ArtReduceInfo;
int  art_get_reduce_info(ArtReduceInfo* out);
/* The stream every later call enqueues on (hipStream_t; NULL = the null stream): art_resize's clears, the whole of a render pass, the
 * read-backs and the device-side updates.  The call itself enqueues nothing and waits for nothing, so work already queued on the stream
 * being left is NOT ordered before work on the new one.  Only art_resize, art_set_shard and the device-side updates (refit, move, rebuild) leave any,
 * since art_render_pass, art_debug_hit_pass and art_download wait at their end: a caller that switches streams after one of those calls
 * art_synchronize first.  Work the CALLER queued on the stream before a library call runs before what that call enqueues. */
int  art_set_stream(void* hip_stream);
int  art_upload_scene(const ArtSceneDesc* scene);        /* Scene.Init: flatten + BVH build + copy to HBM */
int  art_resize(int32_t width, int32_t height);          /* Resize_Viewport (ray_tracer.adb:297-320): zero accum, spp := 0 */
int  art_set_shard(int32_t rank, int32_t nranks, int32_t tile);   /* pixel tiles (tile x tile) dealt along diagonals over the ranks */

/* One Render_Pass.  accum_host (float3 per pixel) and screen_host (u32 per pixel) may be NULL; when given
 * they receive the cumulative accum buffer and the resolved LDR image in p->layout.  *spp_inout is g_spp. */
int  art_render_pass(const ArtPassParams* p, float* accum_host, uint32_t* screen_host, int32_t* spp_inout);

/* Debug_Ray_Tracing + resolve (ray_tracer.adb:208-261).  All pointers optional. */
int  art_debug_hit_pass(const ArtPassParams* p, float* accum_host, uint32_t* screen_host,
                        int32_t* prim_index, int32_t* mat_id, int32_t* prim_type);

/* device-resident variants for the multi-GPU harness: accumulate into caller-owned HBM, e.g. a buffer that is then reduced over xGMI
 * with RCCL.  The binding: the buffer is width*height float3, ROW-MAJOR (pixel (x, y) at floats 3*(y*width + x) ..) whatever p->layout
 * says -- the layout only shapes what the host read-backs hand out.  It must be device memory of the library's device: anything else is
 * refused ("... is not device memory"), nothing is launched and the previous binding stays.  It is not touched at bind time and its
 * size cannot be checked then (the frame may come later): the caller keeps it at least width*height*12 bytes and alive until it is
 * unbound.  art_resize zeroes its first width*height*12 bytes on the library's stream (art_set_stream); every art_render_pass adds its
 * samples into the pixels this rank owns (art_set_shard) and leaves every other pixel as it is, i.e. +0.0f since the resize;
 * art_debug_hit_pass WRITES the debug image into it; art_download and the host pointers of a pass read from it.  art_accum_device()
 * returns it while it is bound, else the library's own buffer (multi-device mode: the reduced frame on device 0).
 * NULL unbinds: the library's own buffer is used again -- it holds what it held before the binding, so call art_resize -- and the
 * caller's buffer is never touched again. */
int  art_bind_accum(void* device_accum_rowmajor);        /* NULL: back to the internal buffer */
/* Luminance moments of the render passes, for a variance-guided denoiser (art_denoise_svgf_device) or an adaptive sampler: caller-owned
 * float2 per pixel, ROW-MAJOR, {S1, S2} at floats 2*(y*width + x).  The rules of art_bind_accum hold: device memory of the library's
 * device, else the call is refused ("... is not device memory") and the previous binding stays; the buffer is not touched at bind time and
 * its size cannot be checked then: the caller keeps it at least width*height*8 bytes and alive until it is unbound.  art_resize zeroes
 * its first width*height*8 bytes on the library's stream; single-device only (refused after art_init_devices(n > 1)); with art_set_shard
 * only the pixels this rank owns are touched, every other pixel stays as it is, i.e. {+0.0f, +0.0f} since the resize.  There is no
 * library-owned moments buffer: NULL (the default) means none, and a pass then launches exactly the kernels it launches without this call.
 * What a pass adds.  One COLOUR of a pixel is one value the pass adds to the accum: with aa_on, background + the four samples of a
 * Generate4RayDirections group, added in the group's order (((bg + s0) + s1) + s2) + s3; without aa_on, one sample.  For every colour
 * (r, g, b) of the pass, in the order in which the colours are added to the accum:
 *   l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;   S1 = l + S1;   S2 = l * l + S2;
 * in binary32, not contracted.  The sums run on over the batches of a pass and over the passes, so they do not depend on how a pass is
 * cut into batches.  A colour that is not finite poisons the pixel's moments for good (NaN or infinity in S1 and S2), as it poisons the
 * pixel's accum.  The number of colours since the resize is n = spp / (aa_on ? 4 : 1); the caller knows it.  art_debug_hit_pass leaves
 * the moments alone.  The accum a pass writes is the same, bit for bit, with and without moments bound. */
int  art_bind_moments(void* device_moments_rowmajor);   /* NULL: none (the default) */
void* art_accum_device(void);
/* Read the framebuffer back (after a reduce in multi-device mode): accum_host and / or screen_host, either may be NULL, in `layout`.
 * The screen is the resolve of the accum as it lies there, whatever wrote it: per channel min((accum * (1.0f / spp)) ** 0.5, 1) * 255
 * rounded to the nearest integer, a tie away from zero, packed R | G << 8 | B << 16; a negative or NaN sum gives 255.  spp is read for
 * the screen only.  With screen_host != NULL, spp <= 0 is refused before anything is launched ("art_download: spp must be positive ..."):
 * the host buffers and the framebuffer stay untouched.  (The reference never resolves at zero samples: Render_Pass counts the pass's
 * samples before it divides.)  With screen_host == NULL any spp is accepted. */
int  art_download(float* accum_host, uint32_t* screen_host, int32_t layout, int32_t spp);
int  art_synchronize(void);

/* Scene.Find_Closest_Hit for a list of rays (host arrays of 3*n floats; tfar may be NULL = unbounded).
 * kernel: 0 = cooperative kernel (bvh_width lanes per ray: 4 by default, 8 as an option), 1 = one-ray-per-lane kernel.  stats may be NULL. */
int  art_trace_rays(const float* origins, const float* dirs, const float* tfar, int64_t n,
                    ArtHit* out, int32_t kernel, ArtStats* stats);

/* Device-resident ray queries (device 0 under art_init_devices).  Every pointer is device memory of the device the library runs on:
 * origins3f / dirs3f are float3 arrays (12 bytes per ray), tnear / tfar one float per ray or NULL (0 / Float'Last, the bound
 * art_trace_rays uses).  n: 0 .. 2^31 - 1, traced in slices of the option "query_slice".  Pointers are checked before anything is
 * launched (host memory or another device's memory: the call fails with art_last_error set).
 * Stream-ordered on hip_stream (NULL: the library's stream, art_set_stream; hipStreamLegacy: the null stream); the host is never made to
 * wait, except when the library's scratch has to grow.  On a stream other than the library's, a query runs after everything the library
 * has enqueued and before anything it enqueues later.
 * Closest hit: with t0 = tnear > 0 ? tnear : 0 (no shift without tnear) the ray traced is o + t0 d, bounded by tfar - t0; an empty interval
 * (!(tfar - t0 > 0)) is a miss.  hits_out[i] is the ArtHit art_trace_rays returns for that ray (byte for byte; a miss holds t = the
 * bound, u = v = 0), except that a hit's t is t0 + t.  kernel: as in art_trace_rays.
 * Occlusion: occluded_out[i] = hits_out[i].is_hit of the closest-hit query on the same ray and interval (the shadow rule's early exit). */
int  art_trace_rays_device(const float* origins3f, const float* dirs3f, const float* tnear, const float* tfar, int64_t n,
                           ArtHit* hits_out, int32_t kernel, void* hip_stream);
int  art_occluded_rays_device(const float* origins3f, const float* dirs3f, const float* tnear, const float* tfar, int64_t n,
                              uint8_t* occluded_out, void* hip_stream);

/* Radiance queries: path-trace rays of the caller's choosing -- "how much light arrives along this ray" -- with the render passes'
 * integrators, stages and trace kernel.  Every pointer is device memory of the device the library runs on: origins3f / dirs3f float3
 * arrays (12 bytes per ray), keys1u one uint32 per ray or NULL, radiance3f float3 per ray, moments2f float2 per ray or NULL.
 * Per-path value.  Ray i is the first ray of `samples` independent paths; path k is what PathTrace (ray_tracer-integrators.adb:82-301,
 *   the integrator render_type selects: ART_PT_STUPID, ART_PT_SHADOW or ART_PT_MIS, to max_depth 1..16) returns for a ray that leaves
 *   origins3f[i] along dirs3f[i].  It starts as a camera sample does: previous pdf 1, previous bounce specular, unbounded -- so a ray that
 *   meets a light face-on returns its emittance (ART_PT_SHADOW: 0, as for a camera ray) and a miss returns 0.  The background colour
 *   plays no part, as it plays none for one sample of a pass without anti-aliasing.
 * RNG key.  The counter-based RNG is keyed by (seed, key_i, sample_base + k, bounce): key_i = keys1u[i], or i when keys1u is NULL; it
 *   stands where a render pass has the pixel index y * width + x.  With the camera rays of a W x H frame without anti-aliasing as the
 *   rays, key_i = i and the frame's spp as sample_base, the path values are those art_render_pass adds to pixel i, bit for bit.
 * Direction.  Used as given: the library does not normalise it (the integrators assume unit length, as camera rays have).
 * Outputs.  radiance3f[3 i ..] is read-modify-write: for k = 0 .. samples - 1 in that order, out = s_k + out per channel, in binary32,
 *   not contracted.  The caller zeroes the buffer first; calling again with sample_base advanced by `samples` refines it, and two calls of
 *   m samples leave the bits one call of 2 m leaves.  The result does not depend on how the call is cut into batches (option
 *   batch_paths).  moments2f, if given, takes the luminance sums of art_bind_moments' formula, one colour being one path value, in the
 *   same order and also read-modify-write:  l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;  S1 = l + S1;  S2 = l * l + S2.
 *   A path value that is not finite poisons its ray's sums, as it poisons a pixel.
 * Refusals, each before anything is launched and with art_last_error set: a null p; a render type other than the three integrators;
 *   max_depth outside 1..16; samples < 1; n outside 0 .. 2^28; (n == 0 then succeeds and launches nothing;) a null origins3f, dirs3f or
 *   radiance3f; no uploaded scene; option trace_kernel = 1 (only the cooperative record schedule has the stages); a pointer that is not
 *   device memory of the library's device or is smaller than n rays need.  Single device: refused after art_init_devices(n > 1).  No
 *   viewport is needed (art_resize); flat and instanced scenes both work.
 * What the call leaves alone: the frame's accum, a bound accum and bound moments, spp, art_get_camera_rays_traced, the shade stage's
 *   items-per-thread trial (the call uses the decided value, as art_render_pass_masked does), ArtStageStats' batches and items, and
 *   ArtStats::samples and pass_ms.  ArtStats::rays, trace_ms and trace_launches DO count the call's rays and trace launches, and
 *   ArtStageStats' stage times its raygen, shade and fold launches; a lost path (ArtStats::lost_paths) fails the call.
 * Stream and waiting.  As art_render_pass_masked: everything runs on the library's stream (art_set_stream) and the call returns when
 *   its work is done, so the outputs are complete on return.  Inputs (rays, keys, and the planes' previous contents) written by work on
 *   ANOTHER stream must be complete before the call: synchronise that stream, or make the library's stream wait for it, first. */
typedef struct ArtRadianceParams {
  int32_t  render_type;   /* ART_PT_STUPID | ART_PT_SHADOW | ART_PT_MIS */
  int32_t  max_depth;     /* 1..16 */
  int32_t  samples;       /* >= 1: paths per ray in this call */
  uint32_t sample_base;   /* RNG sample index of the call's first path */
  uint64_t seed;
} ArtRadianceParams;
int  art_radiance_rays_device(const ArtRadianceParams* p, const float* origins3f, const float* dirs3f, const uint32_t* keys1u /* or NULL */, int64_t n,
                              float* radiance3f, float* moments2f /* or NULL */);

/* First-hit feature buffers of the frame: what a denoiser, a segmentation mask or a compositing step wants
 * next to the radiance.  Every pointer of ArtAovBuffers is device memory of the library's device (device 0 under art_init_devices),
 * row-major (pixel (x, y) at y*width + x) whatever p->layout says; NULL = that plane is not wanted and costs nothing.
 * Frame and scope: the frame art_resize set, always the WHOLE frame on device 0 whatever art_set_shard or art_init_devices dealt, like
 * the device ray queries.  Of p only aa_on and background are read; render_type, max_depth, vthreads, seed and layout are ignored.
 * Rays: pixel q owns K camera rays, K = 4 with aa_on, else 1; ray s is the ray a render pass traces for sample s of q (the
 * Generate4RayDirections offset of s through the camera matrix, from cam_pos, unbounded), traced by the render loop's own trace launch
 * under the option "trace_kernel" as it stands -- the launch art_trace_rays_device uses, so spheres, the Cornell box, rect lights, the
 * REFERENCE_BF mesh and the CLOSEST mesh (or the instances) are all seen.  With h_s the ArtHit art_trace_rays returns for ray s:
 *   hit:   depth_s = h_s.t   normal_s = h_s.normal   albedo_s = albedo of materials[h_s.mat]   hit_s = 1
 *   miss:  depth_s = 0       normal_s = (0, 0, 0)    albedo_s = p->background                  hit_s = 0
 * Albedo of a material: LAMBERT, MIRROR, PHONG p[0..2]; GLASS and LIGHT (1, 1, 1); NULL (0, 0, 0).
 * A float plane holds (((v_0 + v_1) + v_2) + v_3) * 0.25f in binary32, in that association, not contracted (K = 1: v_0); alpha is that
 * mean of hit_s, the normal is not renormalised.  prim_type, prim_index and mat are those of h_0 (-1 on a miss; instanced scenes:
 * prim_index = instance << shift | triangle, as the queries report it).
 * The frame is traced in slices of whole pixels, K * pixels <= the option "query_slice" (at least one pixel), in the queries' scratch.
 * Stream-ordered exactly as art_trace_rays_device: NULL = the library's stream, hipStreamLegacy = the null stream; the host waits only
 * when the scratch has to grow; the call runs after everything the library has enqueued and before anything it enqueues later, so a
 * refit, move or rebuild enqueued before it is seen.  It does not touch the accum buffer, spp, anything a later pass reads of the path
 * state, ArtStageStats or ArtStats: like the device queries' rays, its rays are counted nowhere and its trace launch is not timed.
 * Refused before anything is launched: null p or out, all seven pointers NULL, no scene, no art_resize, a scene committed through
 * gcore_commit_scene (it has no camera), an instanced scene with the option "trace_kernel" 1 (as art_render_pass), and any given
 * pointer that is host memory, another device's memory or too small for its plane. */
typedef struct ArtAovBuffers {
  float*   albedo3f;               /* 3 floats per pixel */
  float*   normal3f;               /* 3 floats per pixel */
  float*   depth;                  /* 1 */
  float*   alpha;                  /* 1: share of the pixel's camera rays that hit anything */
  int32_t* prim_type;              /* ArtHit::prim_type of ray 0, -1 miss */
  int32_t* prim_index;             /* ArtHit::prim_index of ray 0 */
  int32_t* mat;                    /* ArtHit::mat of ray 0 */
} ArtAovBuffers;
int  art_render_aovs_device(const ArtPassParams* p, const ArtAovBuffers* out, void* hip_stream);

/* Feature buffers along rays of the caller's choosing: what art_render_aovs_device gives the built-in
 * pinhole camera, for a camera the caller builds -- a fisheye, a panorama, a thin lens, a lightmap texel grid, a probe grid -- next to the
 * radiance art_radiance_rays_device returns for the same rays.  Every pointer is device memory of the device the library runs on:
 * origins3f / dirs3f float3 arrays (12 bytes per ray), tnear / tfar one float per ray or NULL (0 / Float'Last), the planes of
 * ArtAovRayBuffers one element per GROUP; a NULL plane is not wanted and costs nothing.
 * Grouping.  Rays are group-major: with K = p->group, 1..16, output element g owns rays g*K .. g*K + K - 1; n_rays is a multiple of K.
 *   K stands where a pixel has its 4 anti-aliasing rays.
 * The hit.  h_s is the ArtHit art_trace_rays_device returns for ray s of the group with the same tnear / tfar: its interval rule (the
 *   ray traced is o + t0 d bounded by tfar - t0, an empty interval is a miss, a hit's t is t0 + t'), its trace launch under the option
 *   "trace_kernel" as it stands, and so every kind of primitive: spheres, the Cornell box, rect lights, the REFERENCE_BF mesh, the
 *   CLOSEST mesh or the instances.  The direction is used as given: the library does not normalise it.
 * Per-ray values, with o_s and d_s the ray as the caller gave it:
 *   hit:   depth_s = h_s.t   normal_s = h_s.normal   albedo_s = albedo of materials[h_s.mat]   hit_s = 1   position_s = o_s + h_s.t * d_s
 *   miss:  depth_s = 0       normal_s = (0, 0, 0)    albedo_s = p->background                  hit_s = 0   position_s = (0, 0, 0)
 *   The albedo of a material is art_render_aovs_device's table.  position_s is taken per component in binary32, one multiply then one
 *   add, not contracted.  A sphere's normal is taken at the hit point of the ray's own origin, as h_s.normal is.
 * The float planes (albedo3f, normal3f, position3f, depth, alpha -- alpha is the plane of hit_s) hold
 *   (((v_0 + v_1) + ...) + v_{K-1}) / (float)K:  a left fold in binary32, not contracted, then one correctly rounded division.  K = 1 gives
 *   v_0; K = 4 gives art_render_aovs_device's (...) * 0.25f word for word (a division by 4 is the same exact scaling).
 * The id planes prim_type, prim_index and mat are those of h_0, -1 on a miss; instanced scenes report instance << shift | triangle.
 * With the rays of art_camera_rays_device, group = its K, no bounds and the same background, the seven shared planes are
 *   art_render_aovs_device's, bit for bit.
 * The rays are traced in slices of whole groups, K * groups <= the option "query_slice" (at least one group), in the queries' scratch.
 * Stream-ordered exactly as art_trace_rays_device: NULL = the library's stream, hipStreamLegacy = the null stream; the call runs after
 *   everything the library has enqueued and before anything it enqueues later, so a refit, move or rebuild enqueued before it is seen;
 *   the host waits only when the scratch has to grow.  It touches neither the accum buffer, spp, the path state, ArtStats nor
 *   ArtStageStats, and it needs no viewport (art_resize).
 * Refused before anything is launched, with art_last_error set: a null p or out; all eight planes NULL; group outside 1..16; n_rays
 *   negative, above 2^31 - 1 or not a multiple of group (n_rays == 0 then succeeds and launches nothing); null origins3f or dirs3f; no
 *   uploaded scene; an instanced scene with the option "trace_kernel" 1; a call after art_init_devices(n > 1); any given pointer that is
 *   host memory, another device's memory or too small. */
typedef struct ArtAovRaysParams {
  int32_t group;                   /* K: rays per output element, 1..16 */
  float   background[3];           /* the albedo of a ray that hits nothing */
} ArtAovRaysParams;
typedef struct ArtAovRayBuffers {  /* device memory, one element per GROUP; NULL = not wanted, costs nothing */
  float*   albedo3f;               /* 3 floats per group */
  float*   normal3f;               /* 3 */
  float*   position3f;             /* 3: the mean of the rays' hit points, (0, 0, 0) for a ray that hits nothing */
  float*   depth;                  /* 1 */
  float*   alpha;                  /* 1: share of the group's rays that hit anything */
  int32_t* prim_type;              /* ArtHit::prim_type of ray 0, -1 miss */
  int32_t* prim_index;             /* ArtHit::prim_index of ray 0 */
  int32_t* mat;                    /* ArtHit::mat of ray 0 */
} ArtAovRayBuffers;
int  art_aovs_rays_device(const ArtAovRaysParams* p, const float* origins3f, const float* dirs3f,
                          const float* tnear /* or NULL */, const float* tfar /* or NULL */, int64_t n_rays,
                          const ArtAovRayBuffers* out, void* hip_stream);

/* The frame's own camera rays, into the caller's device memory: what art_render_aovs_device and the render passes trace, for a caller
 * who wants to change them (jitter for depth of field, a crop, a warp) and hand them to art_aovs_rays_device and
 * art_radiance_rays_device.  Of p only aa_on is read.  K = 4 with aa_on, else 1; ray s of pixel q = y*width + x is written at q*K + s:
 * origins3f and dirs3f hold 3 * K * width * height floats each.  The origin is cam_pos; the direction is the one a render pass traces
 * for sample s of q (the Generate4RayDirections offset of s through the camera matrix, normalised): one device function serves all three.
 * Stream-ordered as art_aovs_rays_device; there is no scratch, so the host never waits.  Device 0 under art_init_devices.
 * Refused before anything is launched, where art_render_aovs_device refuses: a null p or a null array, no scene, no art_resize, a scene
 * committed through gcore_commit_scene, a pointer that is host memory, another device's memory or too small. */
int  art_camera_rays_device(const ArtPassParams* p, float* origins3f, float* dirs3f, void* hip_stream);

/* The feature buffers plus a MOTION plane: where each pixel's surface point was one scene update ago, for
 * art_temporal_motion_device to follow geometry that art_refit_device or art_move_instances_device moved.  ONE trace of the camera rays
 * serves all planes: it is art_render_aovs_device's trace, with its slices, its stream rules and its refusals.  out may be NULL, or have
 * all seven pointers NULL, when motion3f is given.  With motion3f NULL the call IS art_render_aovs_device and src is not read.
 * motion3f: device memory, 3 floats per pixel, row-major: the world-space displacement BACK in time of the pixel's surface point -- where
 * the point was, minus where it is.  The caller says what "was" means through ArtMotionSource:
 *   flat scene       cur_pos3f = the vertices in force (what the last art_refit_device, art_rebuild_device or upload put there) and
 *                    prev_pos3f = the vertices one update earlier, both 3 * nverts floats in the uploaded vertex order, both device
 *                    memory; both given or both NULL (NULL: nothing moved).  prev_m12f must be NULL.
 *   instanced scene  prev_m12f = the matrices one update earlier, 12 * n_instances floats as art_move_instances_device takes them; NULL:
 *                    nothing moved.  The vertex pointers must be NULL.  The matrices in force are the library's own (the instance table).
 * The library does NOT check that cur_pos3f is what the tree holds: a wrong array gives a wrong plane and touches nothing else.
 * THE ARITHMETIC (the contract; csrc/art_motion.h is its one definition, compiled for the GPU and for the host).  Binary32, not
 * contracted, in the order written.  T(m, p), row k of a 3 x 4 matrix applied to a point: ((m[4k] * px + m[4k+1] * py) + m[4k+2] * pz) +
 * m[4k+3].  Ray s of the pixel (K = 4 with aa_on, else 1), with h_s its hit record (t, u, v as ArtHit reports them):
 *   a miss, a sphere, a Cornell plane, a rect light, a REFERENCE_BF triangle:   delta_s = (0, 0, 0)
 *   flat scene, CLOSEST triangle i:   (a, b, c) = idx[3i .. 3i + 2];   w = (1.0f - u) - v;   d_k = prev[k] - cur[k] per component of vertex k;
 *       delta_s = (w * d_a + v * d_b) + u * d_c     (u weights C and v weights B, as ArtHit says).  Displacements are interpolated, not
 *       positions: an unmoved (finite) vertex triple gives exactly +0.  Both vertex pointers NULL: delta_s = 0.
 *   instanced scene, triangle of instance j = prim_index >> shift:   Pw = cam_pos + t * d_s per component (d_s the ray's direction);
 *       Po = T(minv_cur[j], Pw);   delta_s = T(prev_m12f[j], Po) - T(m_cur[j], Po) per row, with m_cur and minv_cur record j of the
 *       instance table in force.  A previous matrix equal to the current one word for word gives exactly 0.  prev_m12f NULL: delta_s = 0.
 * The plane holds (((v_0 + v_1) + v_2) + v_3) * 0.25f per component, the association of the other float planes (K = 1: v_0).  A delta
 * that is not finite is stored as it is (art_temporal_motion_device gives such a pixel no history).
 * The flat mesh's index triples are the refit plan's: where no art_refit_device has built the plan since the upload or the last
 * art_rebuild_device, this call builds it as the first refit does, AND THE HOST WAITS for the library's stream that one time.
 * OUT OF SCOPE: a mesh of an instanced scene deformed by art_refit_mesh_device gets the rigid motion of its instance only; what the
 * deformation moved is left to the depth, normal and id tests of the temporal call, as before.
 * Refused before anything is launched, with art_last_error set: everything art_render_aovs_device refuses (but null planes where
 * motion3f is given); motion3f with a null src; only one of cur_pos3f and prev_pos3f; nverts or n_instances other than the uploaded
 * count; vertex arrays on an instanced scene or on a scene without a CLOSEST mesh, matrices on a flat one; any given pointer that is host
 * memory, another device's memory or too small. */
typedef struct ArtMotionSource {
  const float* cur_pos3f;          /* flat scene: the vertices in force, 3 * nverts floats, device memory */
  const float* prev_pos3f;         /* flat scene: the vertices one update earlier, same order, device memory */
  int64_t      nverts;
  const float* prev_m12f;          /* instanced scene: the matrices one update earlier, 12 * n_instances floats, device memory */
  int64_t      n_instances;
} ArtMotionSource;
int  art_render_aovs_motion_device(const ArtPassParams* p, const ArtAovBuffers* out, const ArtMotionSource* src, float* motion3f, void* hip_stream);

/* Edge-avoiding a-trous wavelet denoiser (Dammertz et al. 2010, with the depth-gradient and normal-power edge stops of SVGF), guided by
 * the feature buffers above.  Every pointer is device memory of the library's device (device 0 under
 * art_init_devices), row-major, float3 / float per pixel: the layout of art_bind_accum and ArtAovBuffers.  albedo3f, normal3f and depth
 * may each be NULL: that term is then 1, and without albedo there is no demodulation.  out3f may equal color3f (filtering in place); any
 * other overlap is the caller's error.  The call needs an initialised device only, no scene and no viewport; width and height are the
 * image's own.  It does not touch the accum buffer, spp, ArtStats, ArtStageStats, the path state or the queries' scratch: its scratch is
 * its own (56 bytes per pixel).
 * Stream-ordered exactly as art_render_aovs_device: NULL = the library's stream, hipStreamLegacy = the null stream; the call runs after
 * everything the library has enqueued and before anything it enqueues later; the host waits only when the denoiser's scratch has to grow.
 * Refused before anything is launched, with art_last_error set: null p, color3f or out3f; width or height < 1 or width * height > 2^28;
 * iterations outside 1..8; normal_log2 outside 0..10; variant outside 0..2; a scale that is not finite; a sigma that is NaN; any given
 * pointer that is host memory, another device's memory or too small for its plane.
 *
 * THE ARITHMETIC (the contract; csrc/art_denoise.h is its one definition, compiled for the GPU and for the host).  All operations are
 * binary32, not contracted, in the order written, except where binary64 is named; channel-wise where a colour is meant.  amax(a, b) =
 * (a >= b) ? a : b.  z = depth, n = normal3f, W = width, H = height.
 * Preparation, once per call and pixel:
 *   c_0 = scale * color.   With demodulation (demodulate != 0 and albedo3f given): a = amax(albedo, 1e-3f), c_0 = c_0 / a.
 *   gx = 0.5f * (z(x1, y) - z(x0, y)) with x1 = min(x + 1, W - 1), x0 = max(x - 1, 0); gy likewise in y.
 *   A pixel is BAD IN COLOUR (at iteration i) when a channel of c_i is not finite; BAD IN GUIDES when a given normal component or its
 *   given depth is not finite (albedo does not count).
 * Iteration i = 0 .. iterations - 1, s = 1 << i, centre p = (x, y): acc = 0, wsum = 0; the taps (dx, dy) run with dy = -2..2 outer and
 * dx = -2..2 inner, q = p + s * (dx, dy), and each tap that is not skipped adds, in that order,  acc += w * c_i(q);  wsum += w.
 *   h = k[|dx|] * k[|dy|], k = {0.375f, 0.25f, 0.0625f}.
 *   A tap is skipped when q is outside the image, bad in colour or bad in guides -- the centre tap (dx = dy = 0) too, so a centre that is
 *   bad in colour or in guides does not count itself.  A centre tap that is not skipped has w = h, with no edge terms.  Every other tap:
 *     wn = amax(dot(n_p, n_q), 0.0f), dot = (px * qx + py * qy) + pz * qz, then wn = wn * wn, normal_log2 times.  No normals: wn = 1.
 *     xz = fabsf(z_p - z_q) / (sigma_depth * (fabsf(gx_p * (float)(s * dx)) + fabsf(gy_p * (float)(s * dy))) + (1e-3f * z_p + 1e-6f)).
 *          No depth, or sigma_depth <= 0: xz = 0.
 *     lum(c) = (0.2126f * r + 0.7152f * g) + 0.0722f * b;  xc = fabsf(lum(c_i(p)) - lum(c_i(q))) / (sigma_color * 2^-i)  (2^-i exact).
 *          xc = 0 when sigma_color <= 0 or the centre is bad in colour.
 *     t = -((double)xz + (double)xc);   e = 0.0f when t < -200, else (float)exp_small(t) when t <= 0, else NaN (t is NaN -- a centre bad
 *          in guides, a NaN gradient -- or positive, which only a negative depth can produce).
 *     w = (h * wn) * e;  a w that is NaN skips the tap.
 *     exp_small(t), binary64 throughout: v = t * 0x1.71547652b82fep+0; k = (int)(v + (v >= 0 ? 0.5 : -0.5)) (truncation);
 *          r = (t - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33; q = C13, then q = q * r + C_j for j = 12 .. 0 (Horner), with
 *          C13 .. C0 = 0x1.6124613a86d09p-33, 0x1.1eed8eff8d898p-29, 0x1.ae64567f544e4p-26, 0x1.27e4fb7789f5cp-22, 0x1.71de3a556c734p-19,
 *          0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-13, 0x1.6c16c16c16c17p-10, 0x1.1111111111111p-7, 0x1.5555555555555p-5,
 *          0x1.5555555555555p-3, 0.5, 1.0, 1.0; the result is q * 2^k (csrc/art_math.h m1::exp_small).
 *   c_{i+1}(p) = acc / wsum when wsum > 0, else c_i(p) unchanged (every tap was skipped: the pixel keeps its value, NaN included).
 * After the last iteration: out = c * a with demodulation, else c.
 * So a non-finite colour pixel is never read as a tap and is replaced by its neighbours' weighted mean in the first iteration that
 * reaches a good one.  Quality is not part of the contract; the sigmas' useful range depends on the renderer's units. */
typedef struct ArtDenoiseParams {
  int32_t width, height;     /* the image's own size, row-major; independent of art_resize */
  int32_t iterations;        /* 1..8; iteration i (from 0) uses tap spacing s = 1 << i */
  int32_t demodulate;        /* 1 and albedo given: filter colour / max(albedo, 1e-3f), multiply back at the end */
  int32_t normal_log2;       /* 0..10: normal weight = max(0, n_p . n_q) squared this many times (7 = power 128) */
  int32_t variant;           /* 0 automatic, 1 direct loads, 2 LDS tile: tests and A/B only.  One kernel exists (direct loads): all three select it */
  float   scale;             /* colour is multiplied by this first (1/spp for an accum buffer) */
  float   sigma_color;       /* <= 0: no colour term */
  float   sigma_depth;       /* <= 0: no depth term */
} ArtDenoiseParams;
int  art_denoise_device(const ArtDenoiseParams* p, const float* color3f, const float* albedo3f, const float* normal3f, const float* depth,
                        float* out3f, void* hip_stream);

/* The variance-guided variant of the filter above (the spatial part of SVGF, Schied et al. 2017): the colour
 * stop divides the luminance difference by the local standard deviation of the estimate, which comes from the luminance moments of the
 * render passes (art_bind_moments), instead of by one global constant.  Pointers, layouts, overlap rule (out3f may equal color3f), stream
 * order, scratch (60 bytes per pixel, the same buffer as art_denoise_device's) and the repair of non-finite pixels are those of
 * art_denoise_device.  moments2f: float2 {S1, S2} per pixel, the layout of art_bind_moments; n_colours: the number n of colours the
 * moments hold (spp / 4 with aa_on, else spp).  variance_out: one float per pixel, or NULL; it receives v after the last iteration, the
 * variance of the filtered pixel's luminance in the units the filter works in (scaled, and demodulated when demodulation is on) -- what
 * an adaptive sampler would read.
 * Refused before anything is launched, with art_last_error set: everything art_denoise_device refuses (there is no variant), a null
 * moments2f, n_colours < 2, and a moments2f or variance_out that is host memory, another device's memory or too small for its plane.
 *
 * THE ARITHMETIC (the contract; csrc/art_denoise.h svgf_pack_pixel / svgf_atrous_pixel is its one definition).  The conventions and
 * every symbol not defined here are those of THE ARITHMETIC of art_denoise_device.
 * Preparation, once per call and pixel: c_0, a, gx, gy, BAD IN COLOUR and BAD IN GUIDES exactly as there.  In addition, in binary64
 * (every operand converted first, n = (double)n_colours, each operation rounded to binary64, in the order written):
 *   D = S2 - (S1 * S1) / n;   D0 = (D < 0) ? 0 : D  (a NaN stays a NaN);   v = (D0 * (n / (n - 1))) * (scale * scale);
 *   with demodulation: la = lum(a) (binary32, a the floored albedo), v = v / (la * la).  This is an approximation: the variance of the
 *   luminance of colour / albedo is not the luminance's variance over lum(albedo)^2 unless the albedo is grey.
 *   v_0 = (float)v, the one rounding to binary32.  A v_0 that is not finite becomes +0.0f and marks the pixel NO COLOUR STOP.
 * Iteration i, s = 1 << i, centre p = (x, y):
 *   Variance prefilter: vs = 0, ks = 0; for dy = -1..1 outer, dx = -1..1 inner, q = p + (dx, dy) (spacing 1 in every iteration), each
 *     q that is inside the image, not bad in guides and not bad in colour adds  vs += k * v_i(q);  ks += k;  with k = kk[|dx|] * kk[|dy|],
 *     kk = {0.5f, 0.25f} (so 1/4, 1/8, 1/16).  vg = vs / ks when ks > 0, else 0.0f.
 *   Taps: acc = 0, av = 0, wsum = 0; order, skipping rules, h, wn, xz, t, e, w and exp_small as in art_denoise_device, except
 *     xc = fabsf(lum(c_i(p)) - lum(c_i(q))) / (sigma_color * sqrtf(vg) + 1e-6f), sqrtf correctly rounded; there is no 2^-i factor.
 *     xc = 0 when sigma_color <= 0, the centre is bad in colour or the centre is marked no colour stop.
 *     Each tap that is not skipped adds, in this order,  acc += w * c_i(q);  av += (w * w) * v_i(q);  wsum += w.
 *   c_{i+1}(p) = acc / wsum and v_{i+1}(p) = av / (wsum * wsum) when wsum > 0, else both stay as they were.
 * After the last iteration: out = c * a with demodulation, else c; variance_out = v (not multiplied back).
 * Quality: profiles/svgf/quality.json holds the sweep the defaults of Backend.denoise_svgf_torch were chosen by. */
typedef struct ArtSvgfParams {
  int32_t width, height;     /* the image's own size, row-major; independent of art_resize */
  int32_t iterations;        /* 1..8 */
  int32_t demodulate;        /* as ArtDenoiseParams */
  int32_t normal_log2;       /* 0..10 */
  int32_t n_colours;         /* >= 2: colours behind the moments (art_bind_moments) */
  float   scale;             /* colour is multiplied by this first (1/spp for an accum buffer); v_0 is then the variance of that mean */
  float   sigma_color;       /* <= 0: no colour term; in standard deviations of the pixel's luminance estimate */
  float   sigma_depth;       /* <= 0: no depth term */
} ArtSvgfParams;
int  art_denoise_svgf_device(const ArtSvgfParams* p, const float* color3f, const float* moments2f, const float* albedo3f,
                             const float* normal3f, const float* depth, float* out3f, float* variance_out, void* hip_stream);

/* The same filter fed by a variance plane instead of the moments: what art_temporal_device's variance_out is
 * for, where every pixel has a history length of its own and one n_colours for the frame cannot express it.  variance1f: one float per
 * pixel, row-major, the variance of the pixel's luminance estimate in the units of color3f BEFORE scale.  p->n_colours is ignored.
 * Everything else -- pointers, overlap rule, stream order, scratch, refusals (a null variance1f in place of a null moments2f; no test of
 * n_colours) -- is art_denoise_svgf_device's, and so is THE ARITHMETIC, except for v in the preparation, in binary64:
 *   v = (double)variance1f * ((double)scale * (double)scale);   with demodulation v = v / (la * la) as there;   v_0 = (float)v,
 *   and a v_0 that is not finite (a variance of +infinity: a pixel with fewer than two colours behind it) becomes +0.0f and marks the
 *   pixel NO COLOUR STOP, exactly as there.  Everything after the preparation is the same text (csrc/art_denoise.h svgf_atrous_pixel).
 * Against art_denoise_svgf_device: with variance1f = (float)(D0 * (n / (n - 1))) of that call's own formula the two calls round v twice
 * and once, so their outputs are NOT the same bits in general.  They are when the second rounding is exact: scale a power of two, no
 * demodulation, and neither v nor variance1f subnormal or overflowing (a power-of-two factor commutes with the rounding to binary32). */
int  art_denoise_svgf_var_device(const ArtSvgfParams* p, const float* color3f, const float* variance1f, const float* albedo3f,
                                 const float* normal3f, const float* depth, float* out3f, float* variance_out, void* hip_stream);

/* Temporal reprojection and accumulation, the temporal half of SVGF (Schied et al. 2017): the previous frames'
 * colour and luminance moments are reprojected into the current view by the two cameras and the current depth, checked against depth,
 * normal and id, and blended with the current frame, so that the variance the spatial filter steers by comes from the whole history.
 * Scene-independent like the denoisers: it needs an initialised device only, both cameras arrive in the params, and it touches no accum
 * buffer, spp, ArtStats, ArtStageStats, path state or scratch (it has none: the host never waits).  Stream order and pointer rules are
 * art_denoise_device's: every pointer is device memory of the library's device, row-major; NULL hip_stream = the library's stream.
 * Current frame (cur.width x cur.height): color3f with scale as the denoisers take it; moments2f {S1, S2} and n_colours >= 1 in
 * art_bind_moments' convention; normal3f, depth and id (an int32 plane, e.g. ArtAovBuffers::prim_index or mat) may each be NULL: its test
 * is then passed by every tap, and without depth there is no reprojection (every pixel maps to itself).
 * History: the caller's, one buffer in (hist_in, of the PREVIOUS frame's size prev.width x prev.height; NULL = the first frame, prev is
 * then not read) and one out (hist_out, of the current frame's size), art_temporal_history_bytes(w, h) = 48 * w * h bytes each (0 for a
 * size the call refuses).  They must not overlap: the kernel gathers neighbours.  Layout, for numpy to build and read: three planes of
 * 16-byte records of four binary32 words, plane k at byte 16 * w * h * k, pixel (x, y) at record y * w + x:
 *   plane 0 {r, g, b, n}     the mean colour (scaled) and the history length n in colours, as a float
 *   plane 1 {m1, m2, z, id}  the mean luminance and the mean squared luminance per colour, the frame's depth and id (the int32's bits)
 *   plane 2 {nx, ny, nz, 0}  the frame's normal
 *   (z = +0.0f, id = 0, normal = (0, 0, 0) where the plane is not given).
 * Outputs, each may be NULL: out3f = the blended mean colour (plane 0's r, g, b), length_out = n, variance_out = the variance of that
 * mean's luminance, what art_denoise_svgf_var_device takes (with scale = 1).
 * Refused before anything is launched, with art_last_error set: null p, color3f, moments2f or hist_out; a width or height < 1 or width *
 * height > 2^28 (cur; prev when hist_in is given); n_colours < 1; max_history < n_colours or > 2^24; a scale that is not finite; depth_tol
 * or normal_min NaN; a camera (cur; prev when hist_in is given) with a component that is not finite, with m[3], m[7] or m[11] not zero
 * (camera_dir adds the translation column to a direction, a quirk of the reference no committed scene uses; this call does not follow
 * it) or with a singular 3 x 3; hist_in and hist_out overlapping; any given pointer that is host memory, another device's memory or too
 * small for its plane.
 *
 * THE ARITHMETIC (the contract; csrc/art_temporal.h is its one definition, compiled for the GPU and for the host).  Binary32, not
 * contracted, in the order written, division and sqrtf correctly rounded, except where binary64 is named.  dot(a, b) = (ax * bx + ay * by)
 * + az * bz.  finite(v): neither NaN nor an infinity.  W, H = cur.width, cur.height; Wp, Hp = prev.width, prev.height.
 * Per camera, on the host: cam_z = -(float)width / T with T = safe_tan(pi / 4) = 1.0f exactly (what make_frame computes, art_render.cpp);
 *   M = rows (m[0], m[1], m[2]), (m[4], m[5], m[6]), (m[8], m[9], m[10]) of cam_matrix; its inverse I in binary64 from the binary32
 *   elements: det = (M00 * C00 - M01 * C01) + M02 * C02 with C00 = M11 * M22 - M12 * M21, C01 = M10 * M22 - M12 * M20, C02 = M10 * M21 -
 *   M11 * M20;  I = [ C00, M02 * M21 - M01 * M22, M01 * M12 - M02 * M11;  M12 * M20 - M10 * M22, M00 * M22 - M02 * M20, M02 * M10 - M00 * M12;
 *   C02, M01 * M20 - M00 * M21, M00 * M11 - M01 * M10 ] / det, every product, difference and quotient rounded to binary64, each element
 *   then rounded once to binary32.  Singular: det is zero or not finite, or an element of I is not finite in binary32.
 * Pixel p = (x, y), n_cur = (float)n_colours:
 *  1. c = scale * color;  m1 = S1 / n_cur;  m2 = S2 / n_cur;  z, id, N = the guides (the values above where a plane is not given).
 *  2. The pixel takes NO HISTORY when hist_in is NULL; when depth is given and !(z > 0) (a miss: depth == 0 in the AOV convention) or z is
 *     not finite; when normal3f is given and a component of N is not finite.
 *  3. Where to look.  Without depth, or when prev equals cur word for word (cam_pos, cam_matrix, width, height): fx = (float)x + 0.5f,
 *     fy = (float)y + 0.5f, e = z -- no reprojection, the fractional parts below are exactly 0.  Otherwise:
 *       r = (((float)x + 0.5f) - (float)W / 2.0f, ((float)y + 0.5f) - (float)H / 2.0f, cam_z_cur);   u = (1.0f / sqrtf(dot(r, r))) * r;
 *       t = M_cur u (row k: (Mk0 * ux + Mk1 * uy) + Mk2 * uz);   d = (1.0f / sqrtf(dot(t, t))) * t   -- camera_dir of the pixel centre;
 *       v = (cam_pos_cur + z * d) - cam_pos_prev (per component);   e = sqrtf(dot(v, v));   q = I_prev v (rows as for M);
 *       !(q.z * cam_z_prev > 0): behind the previous camera, NO HISTORY;   k = cam_z_prev / q.z;
 *       fx = q.x * k + (float)Wp / 2.0f;   fy = q.y * k + (float)Hp / 2.0f   (previous-frame coordinates, pixel centres at + 0.5).
 *     With aa_on the AOV depth is the mean of four rays' depths, not the centre ray's: the world point is then an approximation.
 *  4. Gather.  gx = fx - 0.5f, gy = fy - 0.5f;  NO HISTORY unless gx > -1 and gx < (float)Wp and gy > -1 and gy < (float)Hp (a NaN fails).
 *     ix = floorf(gx), ax = gx - floorf(gx), likewise iy, ay.  The taps t = 0..3 in this order: (ix, iy), (ix + 1, iy), (ix, iy + 1),
 *     (ix + 1, iy + 1), with w = wx * wy, wx = ax for the right column and 1.0f - ax for the left, wy likewise.  A tap COUNTS when w > 0;
 *     it is inside the previous frame; its r, g, b, n, m1, m2, z, nx, ny, nz are finite and its n > 0; with depth given,
 *     fabsf(z_tap - e) <= depth_tol * e; with normal3f given, dot(N, N_tap) >= normal_min; with id given, id_tap == id.
 *     Each tap that counts adds, per field of {r, g, b, n, m1, m2}:  sum += w * field;  and  wsum += w.  NO HISTORY unless wsum > 0;
 *     else hist = sum / wsum per field, n_h = hist.n.  (SVGF searches a 3 x 3 neighbourhood when no tap counts; this call does not.)
 *  5. Blend.  NO HISTORY: the pixel becomes its own history, colour c, m1, m2, n = n_cur.  Else cap = (float)max_history - n_cur;
 *     f = (n_h > cap) ? cap / n_h : 1.0f;   n = n_cur + f * n_h;   a = n_cur / n;   b = 1.0f - a;
 *     colour = a * c + b * hist.colour;   m1 = a * m1 + b * hist.m1;   m2 = a * m2 + b * hist.m2.
 *     A colour that is not finite goes into the history as it is; no later frame counts that record as a tap, so the pixel starts again.
 *  6. hist_out: plane 0 {colour, n}, plane 1 {m1, m2, z, id}, plane 2 {N, 0} -- the current frame's guides.  out3f = colour, length_out = n.
 *     variance_out = +infinity where n < 2 (art_denoise_svgf_var_device reads it as "no colour stop"), else in binary64 (operands converted
 *     first): D = m2 - m1 * m1;  D0 = (D < 0) ? 0 : D (a NaN stays);  (float)((D0 * (n / (n - 1))) / n).
 * Reprojection is by camera only: a pixel on a surface that moved fails its depth or id test and starts again
 * (art_temporal_motion_device below follows such a surface).  Quality:
 * profiles/temporal/quality.json holds the sweep the defaults of Backend.temporal_torch were chosen by. */
typedef struct ArtTemporalCamera {
  float   cam_pos[3];
  float   cam_matrix[16];    /* row-major, as ArtSceneDesc::cam_matrix; m[3], m[7], m[11] must be zero */
  int32_t width, height;     /* the frame rendered with this camera */
} ArtTemporalCamera;
typedef struct ArtTemporalParams {
  ArtTemporalCamera cur, prev;   /* prev: read only when hist_in is given */
  int32_t n_colours;         /* >= 1: colours behind color3f and moments2f (spp / 4 with aa_on, else spp) */
  int32_t max_history;       /* n_colours .. 2^24: the history length is capped here, so older frames fade out */
  float   scale;             /* colour is multiplied by this first (1 / spp for an accum buffer) */
  float   depth_tol;         /* a tap's depth may differ from the expected distance by this share of it */
  float   normal_min;        /* least dot product of the two normals */
} ArtTemporalParams;
int  art_temporal_device(const ArtTemporalParams* p, const float* color3f, const float* moments2f, const float* normal3f, const float* depth,
                         const int32_t* id, const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out,
                         void* hip_stream);
int64_t art_temporal_history_bytes(int32_t width, int32_t height);

/* art_temporal_device following moved geometry: the same arguments with motion3f after id -- the plane of
 * art_render_aovs_motion_device for the current frame, 3 floats per pixel, device memory (refused like the other planes when it is host
 * memory, another device's or too small).  With motion3f NULL the call IS art_temporal_device, bit for bit.  With it given, step 3 of THE
 * ARITHMETIC above changes in three places and nowhere else:
 *   - reprojection happens whenever depth and hist_in are given: equal cameras no longer switch it off (without depth there is still no
 *     reprojection, and motion3f is then not read);
 *   - v = ((cam_pos_cur + z * d) + delta) - cam_pos_prev per component, delta = the pixel's three motion floats: the surface point is
 *     taken back to where it was before it is looked up in the previous frame, and e, the distance the tap's depth is held to, follows;
 *   - a pixel whose delta has a component that is not finite takes NO HISTORY.
 * e, q, the behind-the-camera test, the gather, its tests and the blend (the rest of step 3 and steps 4 to 6) stay word for word.  With
 * a delta of zero the call gives art_temporal_device's bits, except between equal cameras: there the old rule skips the projection and
 * this one runs it, so fx, fy come out of the arithmetic and their fractional parts need not be exactly 0.
 * Compulsory traffic: 12 bytes per pixel more than art_temporal_device. */
int  art_temporal_motion_device(const ArtTemporalParams* p, const float* color3f, const float* moments2f, const float* normal3f, const float* depth,
                                const int32_t* id, const float* motion3f, const void* hist_in, void* hist_out, float* out3f, float* variance_out,
                                float* length_out, void* hip_stream);

/* SVGF's spatial variance estimate (Schied et al. 2017, section 4.2): where a pixel's history is short -- the
 * first frame, a disocclusion, a restart on a silhouette -- the variance of art_temporal_device comes from one or two numbers, or is
 * +infinity (fewer than two colours: "no colour stop" in art_denoise_svgf_var_device).  This call replaces it there by the variance of
 * the luminance moments pooled over a (2 * radius + 1)^2 window of the history, weighted by the filter's normal and depth stops, and
 * copies every other pixel's variance.  It goes between art_temporal_device and art_denoise_svgf_var_device.
 * hist: art_temporal_device's hist_out of the frame (48 * width * height bytes, the layout stated there), read only.  variance_in1f,
 * variance_out1f: one float per pixel, row-major; variance_out1f may BE variance_in1f (a pixel reads only its own word of it), it must
 * not overlap hist.  Scene-independent like the denoisers: an initialised device only, no scratch (the host never waits), no ArtStats;
 * stream order and pointer rules are art_temporal_device's.
 * Refused before anything is launched, with art_last_error set: a null pointer; width or height < 1 or width * height > 2^28; radius
 * outside 1 .. 3; normal_log2 outside 0 .. 10; a min_history or sigma_depth that is NaN; variance_out1f overlapping hist; a pointer
 * that is host memory, another device's memory or too small for its plane.
 *
 * THE ARITHMETIC (the contract; csrc/art_svgf_spatial.h is its one definition, compiled for the GPU and for the host).  Binary32, not
 * contracted, in the order written, division correctly rounded, except where binary64 is named.  finite(v): neither NaN nor an infinity.
 * Of pixel q the history holds n_q (plane 0's fourth word), m1_q, m2_q, z_q (plane 1's first three) and the normal N_q (plane 2's first
 * three).  Centre p = (x, y).
 *  LONG HISTORY: n_p >= min_history and finite(variance_in[p]) (a NaN n_p or min_history = +infinity fail):  variance_out[p] =
 *   variance_in[p], the same word.  Nothing else is read for the pixel.
 *  SHORT HISTORY, every other pixel:
 *   Gradient, when sigma_depth > 0 (else 0): gx = 0.5f * (z(x1, y) - z(x0, y)), gy = 0.5f * (z(x, y1) - z(x, y0)) with x1 = min(x + 1,
 *   width - 1), x0 = max(x - 1, 0), likewise y1, y0 -- art_denoise_device's gradient over the history's depth.  zfloor = 1e-3f * z_p + 1e-6f.
 *   Taps: for dy = -radius .. radius outer, dx = -radius .. radius inner, q = p + (dx, dy).  A tap COUNTS when it is inside the frame,
 *   n_q, m1_q, m2_q, z_q and the three words of N_q are finite, n_q > 0, and its weight w is not a NaN.  The centre's w is 1.0f (it
 *   counts under the same tests).  Every other tap: w = wn * e, the normal and depth stops of art_denoise_device, with neither its spline
 *   weight h nor a colour term:
 *     wn = amax(dot(N_p, N_q), 0.0f) squared normal_log2 times (dot and amax as there: (ax * bx + ay * by) + az * bz; a NaN gives 0);
 *     xz = fabsf(z_p - z_q) / (sigma_depth * (fabsf(gx * (float)dx) + fabsf(gy * (float)dy)) + zfloor), or 0.0f when sigma_depth <= 0;
 *     t = -(double)xz;  e = 0.0f when t < -200, (float)exp_small(t) when t <= 0 (exp_small as there), else a NaN (t positive or NaN).
 *   Pooling, in binary64 (operands converted first, each operation rounded to binary64), N = S1 = S2 = 0, per counted tap in that order:
 *     k = w * n_q (exact);   N += k;   S1 += k * m1_q;   S2 += k * m2_q.
 *   N < 2:  variance_out[p] = +infinity.  Otherwise
 *     M1 = S1 / N;   M2 = S2 / N;   D = M2 - M1 * M1;   D0 = (D < 0) ? 0 : D (a NaN stays a NaN);
 *     variance_out[p] = (float)((D0 * (N / (N - 1))) / n_p), the one rounding to binary32 -- the variance of the centre's mean luminance
 *     (n_p as it stands, whatever the centre's own tests said).  A NaN is stored as the quiet NaN 0x7fc00000.
 *   When only the centre counts, N = n_p, M1 = m1_p and M2 = m2_p exactly (k * m1_p is exact in binary64), so the result is step 6 of
 *   art_temporal_device's arithmetic, bit for bit: a window that finds nothing changes nothing.
 * A history made without a normal plane holds N = (0, 0, 0): wn is then 0 for every neighbour and only the centre counts; the same holds
 * for a pixel that missed the scene.  Quality: profiles/svgf_spatial/quality.json holds the sweep the defaults of
 * Backend.svgf_spatial_variance_torch were chosen by. */
typedef struct ArtSvgfSpatialParams {
  int32_t width, height;
  int32_t radius;            /* 1..3; 3 = the 7 x 7 window */
  int32_t normal_log2;       /* 0..10: the normal stop's power, as ArtSvgfParams */
  float   min_history;       /* colours; a pixel with n >= min_history and a finite variance_in keeps variance_in */
  float   sigma_depth;       /* the depth stop, as ArtSvgfParams; <= 0: off */
} ArtSvgfSpatialParams;
int  art_svgf_spatial_variance_device(const ArtSvgfSpatialParams* p, const void* hist, const float* variance_in1f, float* variance_out1f,
                                      void* hip_stream);

/* ---- the display transform ----------------------------------------------------------------------------
 * The tail of the image-space pipeline: a float3 HDR plane in the caller's device memory becomes an exposure (art_auto_exposure_device)
 * and then 8-bit screen words (art_display_device).  Scene-independent like the denoisers: an initialised device only, no viewport, no
 * scratch (the host never waits), no ArtStats; stream order and pointer rules are art_temporal_device's.  color3f is row-major, three
 * floats per pixel, and is only read.
 *
 * THE ARITHMETIC of both calls (the contract; csrc/art_display.h is its one definition, compiled for the GPU and for the host).
 * Binary32, not contracted, in the order written, division and sqrtf correctly rounded, except where binary64 is named; there operands
 * are converted first and every operation is rounded to binary64.  finite(v): neither NaN nor an infinity.  amin(a, b) = (a < b) ? a : b,
 * amax(a, b) = (a >= b) ? a : b, aclamp(v, lo, hi) = amin(amax(v, lo), hi) (a NaN v gives lo).  log_pos, exp_small and apow are ART-M1's
 * (csrc/art_math.h: + - * / in binary64 and one rounding), the functions art_denoise_device and the render passes use.
 *
 * AUTO-EXPOSURE.  state: art_exposure_state_bytes() = 1040 bytes of device memory, 4-byte aligned, that the caller zeroes once:
 *   word 0  float    exposure    the factor art_display_device multiplies by
 *   word 1  float    mean_log2   the trimmed mean of log2 luminance the last counted frame gave
 *   word 2  uint32   counted     pixels of the last call that had a luminance to count (N below)
 *   word 3  uint32   frames      calls so far that counted at least one pixel; 0 = fresh
 *   words 4 .. 259   uint32      the histogram of the last call, bin 0 .. 255
 *  Histogram.  The 256 bin words are set to zero on the stream, then every pixel adds 1 to one bin (integer adds only: per-workgroup
 *  counters in LDS, then integer adds into the state, so the words do not depend on scheduling).  Of pixel p:
 *   r = color[3p] * scale, g, b likewise;   l = (0.2126f * r + 0.7152f * g) + 0.0722f * b      (art_bind_moments' luminance)
 *   not finite(l), or l <= 0:  bin 0 (not counted).  Otherwise, in binary64 throughout (nothing is rounded to binary32):
 *   L = log_pos((double)l) * 0x1.71547652b82fep+0;   t = ((L - min_log2) / (max_log2 - min_log2)) * 254.0;
 *   bin = 1 + (t < 0 ? 0 : t >= 253 ? 253 : (int)floor(t)).      Bin 255 stays 0.
 *  Exposure, one fixed-order walk in binary64 after the histogram.  c_i = bin i's word, i = 1 .. 254; N = their sum (an integer, exact);
 *   a = (double)low_fraction * N;  b = (double)high_fraction * N;  W = S = cum = 0;  for i = 1 .. 254 in turn:
 *     lo = cum;  hi = cum + c_i;  o = (hi < b ? hi : b) - (lo > a ? lo : a);  centre_i = min_log2 + ((i - 1 + 0.5) / 254.0) * (max_log2 - min_log2);
 *     if o > 0:  W += o;  S += o * centre_i.     cum = hi.
 *   (o is the part of bin i's ranks [lo, hi) inside [a, b): a bin that straddles an end is counted in part.)
 *   N == 0 (or W not > 0):  exposure = frames ? exposure : 1.0f;  mean_log2 = frames ? mean_log2 : 0.0f;  counted = 0;  frames stays.
 *   Otherwise:  m = (float)(S / W), the one rounding to binary32;  target = aclamp(key * apow(2.0f, -m), min_exposure, max_exposure);
 *     exposure = frames ? prev + (target - prev) * adapt : target  (prev = the state's exposure);  mean_log2 = m;  counted = N;
 *     frames = frames + 1 (it stops at 2^32 - 1).
 * Refused before anything is launched, with art_last_error set: a null p, color3f or state; width or height < 1 or width * height > 2^28;
 * a scale that is not finite; min_log2 or max_log2 not finite, outside -126 .. 127, or min_log2 >= max_log2; a fraction outside [0, 1] or
 * NaN, or low_fraction >= high_fraction; key, min_exposure or max_exposure not finite or <= 0, or min_exposure > max_exposure; adapt
 * outside (0, 1] or NaN; state overlapping color3f; a pointer that is host memory, another device's memory or too small. */
typedef struct ArtExposureParams {
  int32_t width, height;
  float   scale;               /* the factor on color3f, e.g. 1 / spp for an accum plane */
  float   min_log2, max_log2;  /* the histogram's range of log2 luminance; -12 and 4 */
  float   low_fraction, high_fraction;   /* the ranks of the counted pixels the mean is taken over; 0.5 and 0.95 */
  float   key;                 /* the middle grey the trimmed mean is mapped to; 0.18 */
  float   adapt;               /* (0, 1]: 1 jumps to the target, less moves from the previous exposure towards it by that fraction */
  float   min_exposure, max_exposure;
} ArtExposureParams;
int64_t art_exposure_state_bytes(void);
int  art_auto_exposure_device(const ArtExposureParams* p, const float* color3f, void* state, void* hip_stream);

/* DISPLAY.  One lane per pixel (x, y), p = y * width + x, of the row-major color3f; the pixel's outputs go to element p of screen1u and
 * ldr3f with ART_LAYOUT_ROW_MAJOR and to element x * height + y with ART_LAYOUT_ADA_XY (the constants of art_download).  screen1u (one
 * word per pixel) and ldr3f (three floats per pixel) may each be NULL, not both.  exposure_state: the state of art_auto_exposure_device,
 * whose word 0 is then the exposure (read on the device: no host round trip), or NULL = p->exposure.
 *  ART_CURVE_REFERENCE:  screen = resolve_pixel(color[p], scale), the reference's resolve (ray_tracer.adb:281-291) as art_download runs
 *   it, word for word: exposure, transfer, dither and white are not read, and ldr3f must be NULL (the curve defines screen words only).
 *  Every other curve, per channel c of the pixel:
 *   k = scale * e (e = the exposure; once per pixel);   x = c * k;   not finite(x) or not x > 0:  x = +0;   x = amin(x, 0x1p+60f);
 *   ART_CURVE_LINEAR    v = x
 *   ART_CURVE_REINHARD  v = (x * (1.0f + x / (white * white))) / (1.0f + x)
 *   ART_CURVE_ACES      v = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)
 *   v = aclamp(v, 0.0f, 1.0f);
 *   ART_TRANSFER_SQRT   u = sqrtf(v)
 *   ART_TRANSFER_SRGB   u = (v < 0.0031308f) ? 12.92f * v : 1.055f * apow(v, 0x1.aaaaaap-2f) - 0.055f          (0x1.aaaaaap-2f = 1 / 2.4)
 *   ART_TRANSFER_GAMMA22  u = apow(v, 0x1.d1745ep-2f)                                                           (0x1.d1745ep-2f = 1 / 2.2)
 *   ldr3f receives u.   s = u * 255.0f;
 *   dither 0:  q = ada_round_u32(s) = (s > 0) ? trunc(s) + ((s - trunc(s) >= 0.5f) ? 1 : 0) : 0          (the reference's rounding)
 *   dither 1:  q = trunc(s + ((float)B[y & 3][x & 3] + 0.5f) / 16.0f),  B = {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}}
 *   q = min(q, 255);   screen = q_r | q_g << 8 | q_b << 16.
 *  No input produces anything but 0 .. 255 per channel and a finite u in [0, 1.0000001].
 * Refused before anything is launched, with art_last_error set: a null p or color3f; screen1u and ldr3f both NULL; width or height < 1 or
 * width * height > 2^28; a scale that is not finite; an unknown curve, transfer or layout; dither other than 0 or 1; white not finite or
 * <= 0; without a state an exposure that is not finite or < 0; ldr3f with ART_CURVE_REFERENCE; an output overlapping color3f, the
 * other output or exposure_state (every lane reads the state's first word while others store); a pointer that is host memory, another device's memory or too small. */
enum { ART_CURVE_REFERENCE = 0, ART_CURVE_LINEAR = 1, ART_CURVE_REINHARD = 2, ART_CURVE_ACES = 3 };
enum { ART_TRANSFER_SQRT = 0, ART_TRANSFER_SRGB = 1, ART_TRANSFER_GAMMA22 = 2 };
typedef struct ArtDisplayParams {
  int32_t width, height;
  float   scale;               /* the factor on color3f, e.g. 1 / spp for an accum plane */
  float   exposure;            /* used when exposure_state is NULL */
  int32_t curve;               /* ART_CURVE_... */
  int32_t transfer;            /* ART_TRANSFER_... */
  float   white;               /* the white point of ART_CURVE_REINHARD: x = white maps to 1 */
  int32_t dither;              /* 0: round to nearest; 1: the 4 x 4 ordered dither */
  int32_t layout;              /* ART_LAYOUT_ROW_MAJOR or ART_LAYOUT_ADA_XY, of screen1u and ldr3f */
} ArtDisplayParams;
int  art_display_device(const ArtDisplayParams* p, const float* color3f, const void* exposure_state, uint32_t* screen1u, float* ldr3f,
                        void* hip_stream);

/* ---- bloom: the glare of bright pixels, ahead of the display transform --------------------------------
 * art_display_device clips a light to a flat white disc; the cue for "brighter than white" is the light a lens scatters around such
 * pixels.  This call makes it (Jimenez 2014): the frame is filtered down a pyramid of halved levels, the levels are blended
 * back up into each other, and the result is mixed into the frame.  It goes between the filters and art_auto_exposure_device /
 * art_display_device.  color3f, out3f and bloom3f (each three floats per pixel, row-major; out3f and bloom3f may each be NULL, not
 * both) are device memory of the library's device; exposure_state is the state of art_auto_exposure_device, whose word 0 is then the
 * exposure e (read on the device), or NULL = p->exposure.  out3f may BE color3f: a pixel reads its own words before it writes them and
 * every neighbour is read from the pyramid.  An output that overlaps anything in any other way is refused.  bloom3f receives the
 * scattered light alone.  Scene-independent like the denoisers: an initialised device only, no viewport; the accum buffer, spp,
 * ArtStats and ArtStageStats are not touched.  The pyramid is 16-byte records {r, g, b, +0} in the denoisers' scratch (about 5.4 bytes
 * per frame pixel); stream order and pointer rules are art_firefly_device's: the host waits only when the scratch has to grow.
 *
 * THE ARITHMETIC (the contract; csrc/art_bloom.h is its one definition, compiled for the GPU and for the host).  All operations are
 * binary32, not contracted, in the order written, division correctly rounded; an operation on a texel is that operation on each of its
 * three channels.  finite, amin, amax, aclamp: the display section's (amax(a, b) = (a >= b) ? a : b gives b when a is a NaN, amin
 * likewise).  lum3(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b.  clampi(i, n) = i < 0 ? 0 : i > n - 1 ? n - 1 : i.
 * Read, per channel c of pixel p:   s = scale * c;   not finite(s) or not s > 0:  s = +0;   s = amin(s, 0x1p+60f)      (display's rule).
 *   s(p) is the pixel's three channels after it: finite and not negative for every input, and so is everything below.
 * Prefilter.   threshold == 0 and knee == 0:  L0(p) = s(p), no arithmetic, and the exposure is never read.   Otherwise
 *   l = e * lum3(s(p));    not finite(l) or not l > 0:  f = +0;   otherwise
 *   q = aclamp(l - (threshold - knee), 0.0f, 2.0f * knee);   soft = knee > 0 ? (q * q) / (4.0f * knee) : +0;
 *   c = amax(soft, amax(l - threshold, 0.0f));   f = amin(c / l, 1.0f);         L0(p) = f * s(p)           (the quadratic soft knee)
 * Levels.   w_0 = width, h_0 = height;   w_(k+1) = (w_k + 1) >> 1, h likewise;   levels 1 .. M are made, M = the smaller of `levels`
 *   and the first k >= 1 with w_k = h_k = 1.   D_0 = L0 (never stored).
 * Down, texel (x, y) of level k + 1 from level k:   t[i][j] = D_k(clampi(2 x - 2 + j, w_k), clampi(2 y - 2 + i, h_k)), i, j = 0 .. 5
 *   (i the row);   the quad mean Q(a, b) = ((t[b][a] + t[b][a+1]) + (t[b+1][a] + t[b+1][a+1])) * 0.25f;
 *   inner = (Q(1,1) + Q(3,1)) + (Q(1,3) + Q(3,3));   edge = (Q(2,0) + Q(0,2)) + (Q(4,2) + Q(2,4));   corner = (Q(0,0) + Q(4,0)) + (Q(0,4) + Q(4,4));
 *   D_(k+1)(x, y) = (0.125f * (inner + Q(2,2)) + 0.0625f * edge) + 0.03125f * corner
 *   -- Jimenez's 13 taps: 0.125 centre, 0.125 x 4 inner, 0.0625 x 4 edge, 0.03125 x 4 corner, which sum to 1.
 *   With karis = 1, for k = 0 only, the five boxes of the same quads instead:
 *   g_0 = inner * 0.25f;   g_1 = ((Q(0,0) + Q(2,0)) + (Q(0,2) + Q(2,2))) * 0.25f;   g_2 = ((Q(2,0) + Q(4,0)) + (Q(2,2) + Q(4,2))) * 0.25f;
 *   g_3 = ((Q(0,2) + Q(2,2)) + (Q(0,4) + Q(2,4))) * 0.25f;   g_4 = ((Q(2,2) + Q(4,2)) + (Q(2,4) + Q(4,4))) * 0.25f;
 *   k_0 = 0.5f / (1.0f + lum3(g_0));   k_n = 0.125f / (1.0f + lum3(g_n)), n = 1 .. 4;   K = ((k_1 + k_2) + (k_3 + k_4)) + k_0;
 *   D_1(x, y) = ((((k_1 * g_1) + (k_2 * g_2)) + ((k_3 * g_3) + (k_4 * g_4))) + (k_0 * g_0)) / K     (one hot pixel does not own its box)
 * Up.   up(S, ws, hs)(x, y), the 2 x bilinear rule from a level S of ws x hs texels:   xn = x >> 1;   xf = clampi(x odd ? xn + 1 : xn - 1, ws);
 *   yn, yf likewise with hs;   top = 0.75f * S(xn, yn) + 0.25f * S(xf, yn);   bot = 0.75f * S(xn, yf) + 0.25f * S(xf, yf);
 *   up = 0.75f * top + 0.25f * bot      (an even coordinate lies a quarter past its source texel's near edge: the far one is the one before).
 *   U_M = D_M;   U_k(x, y) = D_k(x, y) + scatter * (up(U_(k+1), w_(k+1), h_(k+1))(x, y) - D_k(x, y)),  k = M - 1 .. 1, in place over D_k.
 * Mix, per pixel p = (x, y):   B = up(U_1, w_1, h_1)(x, y);   bloom3f(p) = B;   out3f(p) = s(p) + strength * (B - s(p)).
 * No atomics and no workgroup waits for another: every texel is a function of the level above or below it alone, so no word depends
 * on scheduling or on `variant`.  strength = 0 gives out3f = s, word for word; with threshold = knee = 0 and karis = 0 the sum of
 * bloom3f is the sum of s up to rounding wherever no level's taps are clamped at an edge (both filters spread every texel with a total
 * weight of 1), and a constant frame of a value with a short mantissa comes out constant.
 * Refused before anything is launched, with art_last_error set: a null p or color3f; out3f and bloom3f both NULL; width or height < 1
 * or width * height > 2^28; levels outside 1 .. 8; karis or variant other than 0 or 1; a scale that is not finite; a threshold or knee
 * that is not finite or < 0; a scatter or strength outside [0, 1] or NaN; without a state an exposure that is not finite or < 0; an
 * output overlapping color3f (other than out3f == color3f), the other output or exposure_state; a pointer that is host memory,
 * another device's memory or too small. */
typedef struct ArtBloomParams {
  int32_t width, height;
  int32_t levels;      /* 1..8 pyramid levels below the frame; levels that would follow a 1 x 1 level are not made */
  int32_t karis;       /* 0 / 1: weight the first downsample's five boxes by 1 / (1 + luminance) so one hot pixel does not flicker */
  int32_t variant;     /* 0: small levels in one workgroup; 1: one launch per level.  Same words either way */
  float   scale;       /* the factor on color3f, e.g. 1 / spp */
  float   exposure;    /* used when exposure_state is NULL; only the threshold reads it */
  float   threshold, knee;   /* soft threshold on exposure * luminance; 0 and 0 = everything scatters (energy conserving) */
  float   scatter;     /* [0, 1]: how much of each coarser level is carried into the finer one on the way up */
  float   strength;    /* [0, 1]: out = s + strength * (bloom - s) */
} ArtBloomParams;
int  art_bloom_device(const ArtBloomParams* p, const float* color3f, const void* exposure_state /* or NULL */,
                      float* out3f /* or NULL */, float* bloom3f /* or NULL */, void* hip_stream);

/* ---- guided upsampling of a low-resolution render ------------------------------------------------------
 * Joint bilateral upsampling (Kopf et al. 2007): a colour plane traced at lo_width x lo_height ("lo") becomes a width x height picture
 * ("hi"), every hi pixel a weighted mean of the lo pixels around it, the weights stopped at edges by feature buffers given at BOTH
 * resolutions (ArtUpsampleGuides: the planes of art_render_aovs_device at the two viewports; id is any of its int32 planes).  With
 * demodulation the lo colour is divided by the lo albedo before the mean and the result multiplied by the hi albedo, so albedo detail
 * comes back at full resolution.  Every pointer is device memory of the library's device, row-major, float3 / float / int32 per pixel;
 * each guide is given on both sides or on neither.  fallback1b (may be NULL): one byte per hi pixel, 0 = the guides reconstructed the
 * pixel, 1 = no tap passed the stops and the pixel is the unguided mean, 2 = no tap had a finite colour and the pixel is black; its
 * non-zero bytes are what art_compact_mask_device selects, for one art_render_pass_masked over the pixels the guides could not fill.
 * The call needs an initialised device only, no scene and no viewport; it does not touch the accum buffer, spp, ArtStats or
 * ArtStageStats.  Its scratch is the denoisers' (32 bytes per lo pixel).  Stream order is art_denoise_device's: NULL = the library's
 * stream, hipStreamLegacy = the null stream; the host waits only when the scratch has to grow.
 *
 * THE ARITHMETIC (the contract; csrc/art_upsample.h is its one definition, compiled for the GPU and for the host).  All operations are
 * binary32, not contracted, in the order written, division correctly rounded, except where binary64 is named.  amax(a, b) = (a >= b) ? a
 * : b.  finite(v): neither NaN nor an infinity.  W, H = width, height; LW, LH = lo_width, lo_height; p = (x, y) a hi pixel, q a lo pixel.
 * Mapping, per hi pixel:
 *   sx = (float)LW / (float)W;   u = ((float)x + 0.5f) * sx - (0.5f + jitter[0]);   i0 = floorf(u);   fx = u - i0.
 *   sy = (float)LH / (float)H;   v = ((float)y + 0.5f) * sy - (0.5f + jitter[1]);   j0 = floorf(v);   fy = v - j0.
 * Taps.  footprint 2: a = 0, 1 with kx(a) = (a == 0) ? 1.0f - fx : fx.   footprint 4: a = -1 .. 2 with the tent
 *   kx(a) = amax(0.0f, 1.0f - fabsf((float)a - fx) / 2.0f).   ky(b) likewise from fy.   h = ky(b) * kx(a) (not normalised: the sum of the
 *   weights is divided out).  The tap (a, b) reads the lo pixel q = (min(max(i0 + a, 0), LW - 1), min(max(j0 + b, 0), LH - 1)): an index
 *   outside the lo frame is clamped to it and keeps its weight.  Its offset from p in hi pixels is that of the unclamped position:
 *   ox = ((float)a - fx) / sx,  oy = ((float)b - fy) / sy.   The taps run with b outer and a inner, each in rising order.
 * Preparation, once per lo pixel:   c(q) = scale * lo_color(q);   with demodulation c(q) = c(q) / amax(albedo_lo(q), 1e-3f).
 *   q is BAD IN COLOUR when a channel of c(q) is not finite; BAD IN GUIDES when a given lo normal component or its given lo depth is
 *   not finite (albedo and id do not count).
 * Of the hi pixel:   n_p, z_p its given normal and depth;   gx = 0.5f * (z(x1, y) - z(x0, y)) with x1 = min(x + 1, W - 1), x0 = max(x - 1,
 *   0), gy likewise in y: art_denoise_device's gradient, over the hi depth.   p is BAD when a given component of n_p or z_p is not
 *   finite, and BACKGROUND when normals are given and n_p == (0, 0, 0) exactly (a miss as art_render_aovs_device writes it).
 * Guided walk (left folds):  acc = 0, wsum = 0; each tap that is not skipped adds, in tap order,  acc += w * c(q);  wsum += w.
 *   A bad p skips every tap.  A tap is skipped when q is bad in colour or bad in guides, or when both id planes are given and
 *   id_lo(q) != id_hi(p).
 *   p background:  a tap counts only where n_q == (0, 0, 0) exactly, with w = h (no normal and no depth term; the id stop stays).
 *   otherwise:  wn = amax(dot(n_p, n_q), 0.0f), dot = (px * qx + py * qy) + pz * qz, then wn = wn * wn, normal_log2 times; no normals: wn = 1.
 *     xz = fabsf(z_p - z_q) / (sigma_depth * (fabsf(gx * ox) + fabsf(gy * oy)) + (1e-3f * z_p + 1e-6f));  no depth, or sigma_depth <= 0: xz = 0.
 *     t = -((double)xz + 0.0);   e = 0.0f when t < -200, else (float)exp_small(t) when t <= 0, else NaN;   w = (h * wn) * e;   a w that is
 *     NaN skips the tap.  This is art_denoise_device's tap weight with no colour term (exp_small as stated there), called, not retyped.
 * Result:   wsum > 0:  out = acc / wsum, fallback 0.   Otherwise the same taps are walked again with w = h, skipping only the taps that
 *   are bad in colour:  wsum > 0:  out = acc / wsum, fallback 1;  else out = (0, 0, 0), fallback 2.
 *   With demodulation out = out * amax(albedo_hi(p), 1e-3f) at the end.
 * With no guide given the result is the plain bilinear (footprint 2) or tent (footprint 4) interpolation of the finite lo pixels.
 * No finite input of moderate size (no overflow of a sum, unit or zero normals, a finite hi albedo) produces a value that is not
 * finite: non-finite lo pixels are never read as taps, and non-finite hi guides lead to the unguided mean.
 * Refused before the device is looked for, with art_last_error set: a null p, lo_color3f, lo, hi or out3f; width or height < 1 or
 * width * height > 2^28; lo_width outside 1 .. width or lo_height outside 1 .. height; footprint other than 2 or 4; normal_log2 outside
 * 0..10; a scale that is not finite; a sigma_depth that is NaN; a jitter outside (-0.5, 0.5) or NaN; a guide given on one side only;
 * demodulate without albedo.  Then: any given pointer that is host memory, another device's memory or too small for its plane; out3f
 * or fallback1b overlapping an input plane or each other. */
typedef struct ArtUpsampleParams {
  int32_t width, height;         /* the output ("hi") frame, row-major */
  int32_t lo_width, lo_height;   /* the input ("lo") frame; 1 <= lo_width <= width, 1 <= lo_height <= height */
  int32_t footprint;             /* 2: the 2 x 2 bilinear taps; 4: 4 x 4 taps under a tent of half-width 2 lo pixels */
  int32_t demodulate;            /* 1 and both albedo planes given: filter colour / albedo_lo, multiply by albedo_hi */
  int32_t normal_log2;           /* 0..10, as ArtDenoiseParams */
  float   scale;                 /* lo colour is multiplied by this first (1/spp for an accum) */
  float   sigma_depth;           /* <= 0: no depth stop */
  float   jitter[2];             /* sub-pixel offset of the lo samples, in lo pixels, each in (-0.5, 0.5) */
} ArtUpsampleParams;
typedef struct ArtUpsampleGuides {   /* device memory; NULL = not given */
  const float* albedo3f; const float* normal3f; const float* depth; const int32_t* id;
} ArtUpsampleGuides;
int  art_upsample_device(const ArtUpsampleParams* p, const float* lo_color3f, const ArtUpsampleGuides* lo, const ArtUpsampleGuides* hi,
                         float* out3f, uint8_t* fallback1b /* or NULL */, void* hip_stream);

/* ---- temporal super-resolution: jittered lo frames accumulated into a hi history -------------------------
 * Each frame is traced at lo_width x lo_height ("lo") with the lo grid moved by a sub-pixel jitter, and every lo sample is put into a
 * history at t.cur.width x t.cur.height ("hi") at the place it was taken: art_temporal_device's accumulation, fed by art_upsample_device's
 * mapping.  Over a few frames every hi pixel has been sampled near its own centre.  lo_color3f and lo_moments2f are the lo frame's colour
 * and luminance moments (art_bind_accum / art_bind_moments at the lo viewport; t.scale and t.n_colours as in art_temporal_device).  The
 * guides (ArtTemporalUpsampleGuides: normal, depth, an int32 id plane) are given at BOTH resolutions or at neither -- the lo ones traced
 * with the jittered camera, the hi ones with the unjittered camera; motion3f is the hi frame's plane of art_render_aovs_motion_device
 * (lo->motion3f must be NULL).  t.cur and t.prev are the UNJITTERED cameras at the HI size.  The histories are art_temporal_device's,
 * word for word, at the hi size (art_temporal_history_bytes(width, height), three planes of 16-byte records): hist_out and variance_out
 * feed art_svgf_spatial_variance_device, art_denoise_svgf_var_device and a later art_temporal_device unchanged.  out3f, variance_out,
 * length_out and fallback1b may each be NULL.  fallback1b: one byte per hi pixel, 0 = filled by counting samples or by the history,
 * 1 = no history and no sample passed the tests, the pixel is the unguided mean of the lo samples around it, 2 = none of them had a finite
 * colour, the record is zero; its non-zero bytes are a mask for art_compact_mask_device / art_render_pass_masked.
 * Scene-independent, stream-ordered like art_upsample_device, no ArtStats.  The call USES LIBRARY SCRATCH (the denoisers', 48 bytes per
 * lo pixel): the host waits only when that scratch has to grow.  Albedo demodulation is NOT in this call: divide the lo colour by the lo
 * albedo before it and multiply out3f by the hi albedo after it.
 * Compulsory traffic: 137 bytes per hi pixel (149 with motion3f) and 136 per lo pixel: 171 per hi pixel at a ratio of 2.
 *
 * THE ARITHMETIC (the contract; csrc/art_temporal_upsample.h is its one definition, compiled for the GPU and for the host).  Binary32,
 * not contracted, in the order written, division and sqrtf correctly rounded, except where binary64 is named.  dot, finite, n_cur and the
 * cameras are art_temporal_device's; amax(a, b) = (a >= b) ? a : b.  W, H = t.cur.width, t.cur.height; LW, LH = lo_width, lo_height.
 * Preparation, once per lo pixel q:  c(q) = scale * lo_color(q);  m1(q) = S1 / n_cur;  m2(q) = S2 / n_cur.  q is BAD IN COLOUR when a
 *   channel of c, m1 or m2 is not finite; BAD IN GUIDES when a given lo normal component or its given lo depth is not finite.
 * Of the hi pixel p = (x, y):  z, id, N = the hi guides (+0.0f, 0, (0, 0, 0) where a plane is not given).  p is BAD when its given depth or
 *   a given normal component is not finite; p is a MISS when depth is given and !(z > 0).
 * A. This frame.
 *   sx = (float)LW / (float)W;  u = ((float)x + 0.5f) * sx - (0.5f + jitter[0]);  i0 = floorf(u);  fx = u - i0;  likewise sy, v, j0, fy
 *   (art_upsample_device's mapping).  The taps t = 0..3 in art_temporal_device's order: (a, b) = (t & 1, t >> 1) at lo pixel
 *   q = (i0 + a, j0 + b).  A tap outside the lo frame is SKIPPED, not clamped.
 *   dx = ((float)a - fx) / sx;  dy = ((float)b - fy) / sy   (the sample's offset from the pixel centre, in hi pixels);
 *   k = amax(0.0f, 1.0f - fabsf(dx) / radius) * amax(0.0f, 1.0f - fabsf(dy) / radius)      (the narrow weight);
 *   h = (a ? fx : 1.0f - fx) * (b ? fy : 1.0f - fy)                                            (the wide weight).
 *   A tap COUNTS when it is inside the lo frame; q is neither bad in colour nor bad in guides; p is not bad; with ids, id_lo(q) == id;
 *   and, for a p that is not a miss: with normals, dot(N, N_lo(q)) >= normal_min; with depth, fabsf(z_lo(q) - z) <= depth_tol * z;
 *   for a p that is a miss, instead of those two: !(z_lo(q) > 0) (a hi miss counts lo misses only).
 *   Left folds in tap order, each from 0:  over the counting taps with k > 0:  K += k;  Ck += k * c(q), likewise M1k, M2k;
 *   over the counting taps with h > 0:  Hs += h;  Ch += h * c(q), likewise M1h, M2h;
 *   over the taps inside the lo frame that are not bad in colour, with h > 0:  Us += h;  Cu += h * c(q), likewise M1u, M2u.
 *   kappa = (K < 1.0f) ? K : 1.0f;   n_eff = kappa * n_cur.   (radius <= min(W / LW, H / LH): the 2 x 2 taps hold every sample the tent
 *   reaches, and K <= 1 up to rounding.)
 * B. History.  art_temporal_device's steps 2 to 4 on the hi guides, t.cur and t.prev, word for word (with motion3f:
 *   art_temporal_motion_device's three changes of step 3): (hist, n_h), or NO HISTORY.
 * C. Combine.
 *   History and K > 0:   c = Ck / K, m1 = M1k / K, m2 = M2k / K;   cap = (float)max_history - n_eff;   f = (n_h > cap) ? cap / n_h : 1.0f;
 *     n = n_eff + f * n_h;   a = n_eff / n;   b = 1.0f - a;   colour = a * c + b * hist.colour;   m1 = a * m1 + b * hist.m1;   m2 likewise
 *     (art_temporal_device's step 5 with n_eff for n_cur).
 *   History and K == 0:  colour, m1, m2 = hist's;   f = (n_h > (float)max_history) ? (float)max_history / n_h : 1.0f;   n = f * n_h.
 *   No history and Hs > 0:   colour = Ch / Hs, m1 = M1h / Hs, m2 = M2h / Hs;   n = n_cur * amax(kappa, min_confidence).
 *   No history, Hs == 0 and Us > 0:   colour = Cu / Us, m1 = M1u / Us, m2 = M2u / Us;   n = n_cur * min_confidence;   fallback = 1.
 *   None of these:   colour, m1, m2, n = 0;   fallback = 2.  (No later frame counts a record with n = 0.)      Otherwise fallback = 0.
 * D. Outputs: art_temporal_device's step 6.  hist_out: plane 0 {colour, n}, plane 1 {m1, m2, z, id}, plane 2 {N, 0} -- the HI guides.
 *   out3f = colour, length_out = n, variance_out = +infinity where n < 2, else the binary64 expression of step 6.
 * With lo size == hi size, jitter 0 and inputs that are finite and pass their own pixel's tests, u = x exactly, only tap (0, 0) has a
 * weight, k = h = 1, and the call gives art_temporal_device's (art_temporal_motion_device's) bits for every radius (a colour of -0.0f
 * comes out as +0.0f: it went through 0 + 1 * c).
 * Refused before anything is launched, with art_last_error set: a null p, lo_color3f, lo_moments2f, lo, hi or hist_out; a guide given on
 * one side only; lo->motion3f not NULL; everything art_temporal_device refuses for t at the hi size (with hi->motion3f as the motion
 * plane); lo_width outside 1 .. width or lo_height outside 1 .. height; a jitter outside (-0.5, 0.5) or NaN; radius outside
 * (0, min((float)W / (float)LW, (float)H / (float)LH)] or NaN; min_confidence outside (0, 1] or NaN.  Then: any given pointer that is host
 * memory, another device's memory or too small for its plane; an output overlapping an input plane or another output. */
typedef struct ArtTemporalUpsampleGuides {   /* device memory; NULL = not given */
  const float* normal3f; const float* depth; const int32_t* id; const float* motion3f;
} ArtTemporalUpsampleGuides;
typedef struct ArtTemporalUpsampleParams {
  ArtTemporalParams t;        /* cur / prev: the UNJITTERED cameras at the HI size; n_colours, max_history, scale, depth_tol, normal_min as in art_temporal_device */
  int32_t lo_width, lo_height;
  float   jitter[2];          /* offset of this frame's lo samples, in lo pixels, inside (-0.5, 0.5): art_upsample_device's convention */
  float   radius;             /* half-width in HI pixels of the tent a lo sample is splatted with */
  float   min_confidence;     /* in (0, 1]: the history length, as a share of n_colours, of a pixel filled without history */
} ArtTemporalUpsampleParams;
int  art_temporal_upsample_device(const ArtTemporalUpsampleParams* p, const float* lo_color3f, const float* lo_moments2f,
                                  const ArtTemporalUpsampleGuides* lo, const ArtTemporalUpsampleGuides* hi,
                                  const void* hist_in /* or NULL */, void* hist_out, float* out3f, float* variance_out, float* length_out,
                                  uint8_t* fallback1b, void* hip_stream);

/* ---- firefly suppression ahead of temporal accumulation ------------------------------------------------
 * A path that finds the light through a specular chain puts one pixel far above its neighbours; blended into a history it glows for
 * max_history frames and inflates the variance the filters are guided by.  This call takes such outliers out of the FRAME, before
 * art_temporal_device: a pixel whose luminance exceeds a limit made from the rank-th largest luminance among its neighbours is scaled
 * down to that limit, its moments with it.  It goes between the render pass and art_temporal_device / art_temporal_upsample_device.
 * color3f (3 floats per pixel), moments2f ({S1, S2} per pixel in art_bind_moments' convention, or NULL), id (an int32 plane, e.g.
 * ArtAovBuffers::prim_index, or NULL: every neighbour counts), out3f, moments_out2f (NULL if and only if moments2f is NULL) and
 * clamped1b (one byte per pixel, or NULL): row-major device memory of the library's device.  out3f may BE color3f and moments_out2f
 * may BE moments2f (the same address): the window reads a key plane in the library's scratch, never the colour, and a pixel reads its
 * own words before it writes them.  An output plane that overlaps any other plane in any other way is refused.
 * The call needs an initialised device only, no scene and no viewport; it does not touch the accum buffer, spp, ArtStats or
 * ArtStageStats.  Its scratch is the denoisers' (4 bytes per pixel).  Stream order is art_denoise_device's: NULL = the library's
 * stream, hipStreamLegacy = the null stream; the host waits only when the scratch has to grow.
 *
 * THE ARITHMETIC (the contract; csrc/art_firefly.h is its one definition, compiled for the GPU and for the host).  All operations are
 * binary32, not contracted, in the order written, division correctly rounded.  amax(a, b) = (a >= b) ? a : b.  finite(v): neither NaN
 * nor an infinity.  lum3(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b, the filters' luminance.  QNAN = the word 0x7fc00000.
 * Key, per pixel q:   c(q) = scale * color(q) per channel;   l(q) = lum3(c(q)).   q is BAD when a channel of c(q) or l(q) is not
 *   finite.   key(q) = l(q), or QNAN for a bad pixel.
 * Neighbours of p = (x, y):   the q = (x + dx, y + dy) with |dx| <= radius, |dy| <= radius, q != p, that lie inside the frame and are
 *   not bad; with id given only those with id(q) == id(p).   count = how many there are.
 * Limit:   m = the rank-th largest of the neighbours' keys (equal keys each take a place; it is a function of the values alone, so no
 *   order of visiting changes it; -infinity when count < rank, which min_count keeps from being used).
 *   T = amax(gain * m + (floor + 0.0f), 0.0f)    (the + 0.0f makes a floor of -0.0f a +0.0f: T never carries the sign of a zero key).
 * Result:
 *   p bad:                                   out = c(p),  moments_out = moments,  clamped = 2   (the later calls repair such pixels)
 *   count < min_count,  or  !(l(p) > T):     out = c(p),  moments_out = moments,  clamped = 0
 *   otherwise:   f = T / l(p);   out = f * c(p) per channel;   moments_out = (f * S1, (f * f) * S2);   clamped = 1
 *     -- every sample of the pixel scaled by f, so art_temporal_device sees moments consistent with the colour it is given.
 *   "moments_out = moments" copies the two words as they are.  Every word of out3f that is a NaN, and every word of moments_out2f
 *   that is computed (clamped = 1) and is a NaN, is stored as QNAN (processors differ in the sign and payload they give one).
 * Since l(p) > T >= 0 at a clamped pixel, 0 <= f < 1: no finite input produces an output that is not finite, and the call never
 * raises a value.  A frame of equal keys is left alone at gain 1 (l > T is false), and so is a black frame at floor 0.
 * The non-zero bytes of clamped1b are what art_compact_mask_device selects: one art_render_pass_masked over the clamped (and bad)
 * pixels gives them more samples where that is wanted.  out3f holds the SCALED colour: the calls after this one take scale = 1.
 * Refused before the device is looked for, with art_last_error set: a null p, color3f or out3f; moments_out2f given without moments2f
 * or moments2f without moments_out2f; width or height < 1 or width * height > 2^28; radius other than 1 or 2; rank outside 1 .. 4;
 * min_count outside rank .. (2 * radius + 1)^2 - 1; a scale that is not finite; a gain that is not finite or below 1; a floor that is
 * not finite or below 0.  Then: any given pointer that is host memory, another device's memory or too small for its plane; an output
 * plane overlapping another plane (other than out3f == color3f and moments_out2f == moments2f). */
typedef struct ArtFireflyParams {
  int32_t width, height;
  int32_t radius;            /* 1 or 2: the 3 x 3 or the 5 x 5 window */
  int32_t rank;              /* 1..4: the limit comes from the rank-th largest neighbour (2 lets one neighbouring firefly pass) */
  int32_t min_count;         /* rank .. (2 * radius + 1)^2 - 1: a pixel with fewer neighbours is left alone */
  float   scale;             /* colour is multiplied by this first (1 / spp for an accum buffer) */
  float   gain;              /* finite, >= 1: how far above the rank-th neighbour a pixel may stand */
  float   floor;             /* finite, >= 0: added to the limit, so dark surroundings do not clamp to black */
} ArtFireflyParams;
int  art_firefly_device(const ArtFireflyParams* p, const float* color3f, const float* moments2f /* or NULL */, const int32_t* id /* or NULL */,
                        float* out3f, float* moments_out2f /* NULL iff moments2f is NULL */, uint8_t* clamped1b /* or NULL */,
                        void* hip_stream);

/* ---- adaptive sampling ------------------------------------------------------------------------------
 * Three calls: a byte mask over the frame is compacted into a pixel list, a render pass runs over the pixels of a mask only, and one
 * kernel turns accum, moments and per-pixel sample counts into the mean, its variance, a relative error and the next mask.
 *
 * Ordered stream compaction of a mask over this rank's pixel list.  mask1b: one byte per pixel of the art_resize frame, row-major, device
 * memory; non-zero = selected.  With pixmap[0 .. npix_local) the rank's pixel list (art_set_shard; 32 x 32 tiles, tile after tile, rows
 * inside a tile: csrc/art_host_scene.cpp build_pixmap), pixels_out receives the global pixel indices g = pixmap[i] (y * width + x) with
 * mask1b[g] != 0, for i = 0 .. npix_local - 1 IN THAT ORDER -- the list a render pass walks, filtered, so a masked pass keeps the tile
 * locality of a full one -- and *count_out (one device word) their number.  Words of pixels_out from *count_out on are not written.  The
 * result is the same bytes on every run: three launches (per-workgroup counts, a scan of those counts, the scatter), no atomic decides
 * a position and no workgroup waits for another.  cap: the words pixels_out holds.
 * Stream-ordered exactly as art_render_aovs_device (NULL = the library's stream, hipStreamLegacy = the null stream; the call runs after
 * everything the library has enqueued and before anything it enqueues later; the host waits only when the library's scratch of one word
 * per 256 list entries has to grow); under art_init_devices it is device 0's list.  Refused before anything is launched, with
 * art_last_error set: a null pointer, no art_resize, a list of more than 2^28 pixels, cap smaller than the rank's list (npix_local), any
 * pointer that is host memory, another device's memory or too small (width * height bytes of mask, 4 * cap of pixels_out, 4 of count_out). */
int  art_compact_mask_device(const uint8_t* mask1b, uint32_t* pixels_out, int64_t cap, uint32_t* count_out, void* hip_stream);

/* One Render_Pass over the selected pixels of this rank's list: art_render_pass restricted to mask1b (device memory, a byte per pixel of
 * the frame, row-major, non-zero = selected).  The mask is compacted (as art_compact_mask_device does) into a list the library owns,
 * THE HOST WAITS for the library's stream ONCE to read the list's length back (4 bytes: it plans the batches), and the pass then runs
 * art_render_pass's batches over that list.  The RNG is keyed by pixel, sample index and bounce, so:
 *   - the samples are those with indices spp .. spp + S - 1 (S = vthreads * (aa_on ? 4 : 1), spp = *spp_inout as art_render_pass reads
 *     it), and *spp_inout advances by S WHATEVER the mask holds, also when it selects nothing;
 *   - a selected pixel this rank owns receives exactly the colours the full pass at that spp would add, in the same order, into the accum
 *     (the library's or art_bind_accum's) and into bound moments: bit for bit the full pass restricted to the mask;
 *   - no word of any other pixel's accum or moments is written.
 * The frame's pixels then no longer share one sample count.  counts1u (may be NULL): a caller-owned uint32 per pixel, row-major, device
 * memory; a kernel of its own adds S to the word of every selected pixel this rank owns.  art_resize does not know the buffer: the caller
 * zeroes it (and adds S itself after a full pass).  ArtStats::samples grows by (selected pixels) * S; rays and the stage statistics come
 * out of the kernels as ever.  *pixels_out (may be NULL, host memory) = the number of selected pixels this rank owns.
 * The shade stage's items-per-thread trial (option "shade_per" = 0) is neither advanced nor reset: a masked pass runs with the pinned
 * option, else the decided value, else 4, and a later full pass behaves as if the masked one had not happened.  The picture never
 * depends on that setting.  The call ends as art_render_pass does: it waits for the pass and reports lost paths.
 * Refused before anything is launched (the accum, *spp_inout and counts1u stay as they were): everything art_render_pass refuses; a null
 * mask1b; art_init_devices(n > 1) (as art_bind_moments); a mask1b or counts1u that is host memory, another device's memory or too small. */
int  art_render_pass_masked(const ArtPassParams* p, const uint8_t* mask1b, uint32_t* counts1u, int32_t* spp_inout, int64_t* pixels_out);

/* Per pixel: the mean colour, the variance of the mean's luminance, a relative error and the mask of the next masked pass, in one kernel
 * (one lane per pixel).  Scene-independent like the denoisers: it needs an initialised device only and touches no accum buffer, spp,
 * ArtStats, path state or scratch (it has none: the host never waits).  Stream order and pointer rules are art_temporal_device's.
 * Inputs, device memory, row-major: accum3f (art_bind_accum's layout), moments2f {S1, S2} (art_bind_moments), counts1u = the samples
 * behind each pixel (art_render_pass_masked).  Outputs, each may be NULL but not all: mean3f (3 floats), variance1f, error1f (1 float),
 * mask1b (1 byte, 0 or 1).  mean3f may be accum3f itself; any other overlap is the caller's error.
 * Refused before anything is launched, with art_last_error set: null p, accum3f, moments2f or counts1u; all four outputs NULL; width or
 * height < 1 or width * height > 2^28; min_colours < 2; max_samples < 0; a threshold that is NaN; a lum_floor that is negative or not
 * finite; any given pointer that is host memory, another device's memory or too small for its plane.
 *
 * THE ARITHMETIC (the contract; csrc/art_adaptive.h is its one definition, compiled for the GPU and for the host).  Pixel q.  Except for
 * the mean, operands are converted to binary64 first, every operation is rounded to binary64 in the order written (division and sqrt
 * correctly rounded), and each stored float is rounded ONCE to binary32.
 *   per = aa_on ? 4 : 1;   s = counts1u[q];   n = s / per (the colours: a quotient in binary64);   k = 1 / per.
 *   mean3f = (1.0f / (float)s) * accum3f, channel-wise in binary32;  s = 0: mean3f = +0.0f.
 *   s = 0 or n < 2:  variance1f = error1f = +infinity (art_denoise_svgf_var_device reads that as "no colour stop").
 *   Otherwise, with S1, S2 the pixel's moments:
 *     D = S2 - (S1 * S1) / n;   D0 = (D < 0) ? 0 : D (a NaN stays a NaN);   v = (D0 * (n / (n - 1))) / n;   m = (S1 / n) * k;
 *     variance1f = (float)(v * (k * k))   -- the variance of the mean's luminance in the units of mean3f: what
 *                                            art_denoise_svgf_var_device takes with scale = 1;
 *     error1f = (float)((sqrt(v) * k) / (fabs(m) + lum_floor))   -- the standard error of the mean's luminance relative to it.
 *     A variance1f or error1f that is a NaN is stored as the quiet NaN 0x7fc00000, whatever sign and payload the arithmetic gave it
 *     (processors differ there); mean3f keeps what the binary32 product gives.
 *   mask1b = (s < max_samples) && (n < min_colours || !(error1f <= threshold)) ? 1 : 0, the comparison on the stored binary32 error:
 *   an error equal to the threshold is converged, a NaN error keeps the pixel selected until s reaches max_samples, and a zero counts
 *   plane selects every pixel (with max_samples > 0).
 * Quality: profiles/adaptive/quality.json holds the sweep the defaults of Backend.render_adaptive were chosen by. */
typedef struct ArtAdaptiveParams {
  int32_t width, height;
  int32_t aa_on;             /* the passes' anti-aliasing: a colour is 4 samples with it, else 1 */
  int32_t min_colours;       /* >= 2: a pixel with fewer colours is always selected */
  int32_t max_samples;       /* >= 0: a pixel with this many samples is never selected */
  float   threshold;         /* error1f <= threshold: the pixel is converged */
  float   lum_floor;         /* >= 0, added to |mean luminance| in the error's denominator: dark pixels are not chased */
} ArtAdaptiveParams;
int  art_adaptive_estimate_device(const ArtAdaptiveParams* p, const float* accum3f, const float* moments2f, const uint32_t* counts1u,
                                  float* mean3f, float* variance1f, float* error1f, uint8_t* mask1b, void* hip_stream);

/* The camera of the uploaded scene: cam_pos and cam_matrix replace ArtSceneDesc's in every context under
 * art_init_devices, without a rebuild.  Stream-ordered on the library's stream (art_set_stream), like the other scene updates: work
 * enqueued before the call sees the old camera, work enqueued after it the new one.  Every later pass, AOV call and query gives, bit for
 * bit, what a fresh art_upload_scene of the same scene with that camera gives.  What follows the camera: the scene header (the host's
 * copy the kernels take at launch, and the copy in HBM), and on an instanced scene the scene's extent -- the largest |coordinate| a ray
 * can start at, the camera's included -- which the absolute pad of every mesh's boxes follows.  Pads only grow, as for
 * art_move_instances_device: a camera inside the extent the pads were made for changes the header alone and the host never waits; a
 * camera OUTSIDE it raises the extent and re-pads at the matrices in force by the kernels of a move (its re-pads count in
 * ArtMoveInfo::repads), and the host waits only where that builds the plan a move shares (the first update after an upload).  The flat
 * mesh's tree, the spheres, lights, materials, the pixel tiles and the path state do not depend on the camera.
 * Refused before anything changes, with art_last_error set: no scene, a scene committed through gcore_commit_scene, a null pointer, a
 * component that is not finite. */
int  art_set_camera(const float cam_pos[3], const float cam_matrix[16]);

/* Moving geometry.  Moves the vertices of the scene's ART_MESH_CLOSEST mesh and refits its tree in place: same
 * topology, same leaf order, new boxes (the builders' padding rule, quantised again at width 4), for every builder and both widths.
 * pos3f: device memory, 3*nverts floats, in the vertex order of the ArtMesh.pos uploaded; nrm3f: the same for normals, or NULL = keep
 * them.  Material ids stay.  Stream-ordered like art_trace_rays_device (NULL = the library's stream; hipStreamLegacy: the null stream):
 * work enqueued before the call sees the old geometry, work enqueued after it the new; the host waits only on the first call after an
 * upload, which builds the refit plan (the nodes grouped by depth) and its scratch.  Under art_init_devices every context is refitted,
 * the others from a peer copy of pos3f / nrm3f (device 0 memory).  Refused before anything is launched: no scene, an instanced scene,
 * no CLOSEST mesh, a scene committed through gcore_commit_scene, nverts other than the uploaded count, host memory or another device's
 * memory.  A vertex coordinate that is not finite or whose magnitude exceeds 1e18 empties every box holding it (no ray enters it) and
 * makes the next art_synchronize fail with the count; a later good refit or an upload clears that state.  The tree keeps the topology
 * it was built with: after large deformations traversal costs more (art_get_tree_cost says how much), and art_rebuild_device builds a
 * new tree without leaving the GPU (art_upload_scene does it through the host). */
int  art_refit_device(const float* pos3f, const float* nrm3f, int64_t nverts, void* hip_stream);
/* Cumulative since art_upload_scene (waits for the refits enqueued so far): refit_ms = HIP events around device 0's refit kernels,
 * plan_ms = host time of building the refit plans, bad_vertices = bad vertex coordinates counted on device 0 over all refits. */
typedef struct ArtRefitInfo { uint64_t refits; double refit_ms; double plan_ms; uint64_t bad_vertices; } ArtRefitInfo;
int  art_get_refit_info(ArtRefitInfo* out);

/* A new tree for the moved mesh, built on the GPU.  The arguments are art_refit_device's: device memory of the
 * library's device, in the vertex order of the uploaded ArtMesh.pos; nrm3f == NULL keeps the normals; material ids stay.  The tree is the
 * one the next art_upload_scene of the same mesh at these positions would build under the options as they stand at the call (bvh_width,
 * bvh_builder, bvh_max_leaf, the cost options, bvh_ploc_radius): byte for byte with builder 3, the same tree from the GPU binned-SAH
 * builder with builder 0, a tree whose node numbering may differ from one build to the next with builders 1 and 2.  Nothing goes through
 * the host: the corners are gathered in HBM, every context builds into new buffers, and only the tree, its padded triangle copy and (with
 * nrm3f) the normals of the shading records are replaced -- no other array of the scene is touched.
 * Work already enqueued on hip_stream and on the library's stream runs before the rebuild; work enqueued afterwards sees the new
 * geometry.  UNLIKE A REFIT THE CALL RETURNS ONLY WHEN THE NEW TREE IS COMMITTED: the builders size their output from counts they read
 * back, level by level, so the host waits for hip_stream and for the library's stream.
 * Refused before anything is launched: everything art_refit_device refuses (no scene, an instanced scene, no CLOSEST mesh, a scene
 * committed through gcore_commit_scene, a wrong nverts, host memory or another device's memory), the option bvh_spatial_splits (reference
 * splitting exists in the host builder only), and a mesh of fewer than two triangles (it has no GPU-built tree; refit it).  Bad vertices
 * (the refit's rule: not finite, or beyond 1e18 in magnitude) are counted by the gather kernel and the count is read before a builder
 * starts: the call fails with the count.  A rebuild that fails (a bad vertex, the allocator, a builder, a traversal-stack bound above
 * kStackEntries, the limit art_upload_scene applies) leaves the scene of every context exactly as it was: every context builds into
 * new buffers, and everything that can fail on a working device happens before the first context swaps.  The swap itself copies one
 * header per context and launches one kernel for the normals; it fails only when a device is lost, the one case in which the contexts
 * of art_init_devices may be left with different trees.  A failed call is not counted in ArtRebuildInfo.  A successful one clears a
 * bad refit's state and drops the refit plan; the next art_refit_device plans against the new tree.  Under art_init_devices every
 * context is rebuilt from a peer copy. */
int  art_rebuild_device(const float* pos3f, const float* nrm3f, int64_t nverts, void* hip_stream);
/* Cumulative since art_upload_scene: gather_ms = HIP events around device 0's gather kernel, build_ms = HIP events around device 0's
 * builds (ArtBvhInfo::build_ms of each), host_ms = host time inside art_rebuild_device (all contexts, commit included). */
typedef struct ArtRebuildInfo { uint64_t rebuilds; double gather_ms; double build_ms; double host_ms; } ArtRebuildInfo;
int  art_get_rebuild_info(ArtRebuildInfo* out);   /* cumulative since art_upload_scene */

/* How good is the tree in HBM right now (device 0; waits for the library's stream): the surface-area expectation of the work of a random
 * line through the root, from the binary32 child boxes the walk tests (at width 4 the dequantised tree).  With A(box) the half surface
 * area in binary64: root_area = A(union of the root's used child boxes), node_visits = 1 + sum over inner child slots of A / root_area,
 * leaf_visits = sum over leaf slots of A / root_area, tri_tests = sum over leaf slots of count * A / root_area.  An empty slot adds
 * nothing, nor does one a bad-vertex refit emptied.  A caller compares the figure of a refitted tree with that of a rebuilt one to
 * decide when to rebuild; the library sets no policy.  Fails without a scene, on an instanced scene, and on a scene without a tree. */
typedef struct ArtTreeCost { double root_area, node_visits, leaf_visits, tri_tests; } ArtTreeCost;
int  art_get_tree_cost(ArtTreeCost* out);   /* device 0; waits for the library's stream */

/* Moving the instances of an instanced scene.  m12f: device memory of the library's device, 12*n_instances
 * floats: instance i's object -> world 3x4, row-major, in the order of ArtSceneDesc::instances.  Which mesh an instance shows and
 * everything about the meshes stay as uploaded.  Kernels rewrite the instance table (m, and the inverse in invert_3x4's arithmetic:
 * the bytes an upload would write), the world box and proxy record of every entry point (the upload's tight box), the instance tree's
 * boxes (its topology, its entry points and the inst_open choice stay as built) and -- because the absolute pad of a mesh's boxes
 * follows the inverse matrices of its instances -- the boxes of every mesh whose pad the new placement outgrows.  Pads only grow: a
 * mesh's boxes are never narrower than an upload at the new transforms would make them.  Picture, ray count and hit records are those
 * of art_upload_scene at the new transforms, bit for bit.  Stream-ordered exactly as art_refit_device is: work enqueued before the
 * call sees the old placement, work enqueued after it the new one; the host waits only on the first call after an upload, which
 * builds the plan.  Under art_init_devices every context is moved, the others from a peer copy of m12f.  Refused before anything is
 * launched: no scene, a scene committed through gcore_commit_scene, a scene that is not instanced, n_instances other than the
 * uploaded count, host memory or another device's memory.  A matrix with an element that is not finite, whose determinant fails
 * the upload's test, or that places a coordinate of its mesh's box beyond 1e18 in magnitude (art_refit_device's limit for a vertex
 * coordinate; the boxes are quantised by a loop that needs finite input) is a bad matrix: every entry point of its instance gets an empty box (no ray enters it) and the next
 * art_synchronize fails with the count; a later good move or an upload clears that state.  After instances have travelled far the
 * instance tree costs more to walk than the one a fresh art_upload_scene builds. */
int  art_move_instances_device(const float* m12f, int64_t n_instances, void* hip_stream);
/* moves = calls accepted, move_ms = HIP events around device 0's move kernels, plan_ms = host time of building the plans,
 * bad_matrices = bad matrices counted on device 0 over all moves, repads = meshes whose boxes were re-padded, over all moves. */
typedef struct ArtMoveInfo { uint64_t moves; double move_ms; double plan_ms; uint64_t bad_matrices; uint64_t repads; } ArtMoveInfo;
int  art_get_move_info(ArtMoveInfo* out);   /* cumulative since art_upload_scene; waits for the moves enqueued so far */

/* Deforming a mesh of an instanced scene.  mesh indexes ArtSceneDesc::meshes of the uploaded instanced scene;
 * pos3f / nrm3f: device memory of the library's device, 3*nverts floats in the vertex order of that ArtMesh, in object space; nrm3f ==
 * NULL keeps the normals.  Indices, material ids, which mesh an instance shows and the matrices stay.  Kernels rewrite the mesh's
 * triangle records, their padded copy and (with nrm3f) its shading records, refit the mesh's tree level by level (its topology and leaf
 * order stay; the entry points stay where the build opened them), and then bring everything that depends on where the triangles are up
 * to date at the matrices in force (the uploaded ones, or the last accepted move's): the absolute pads of the meshes' boxes -- the
 * scene's extent follows the mesh's box, so a mesh that grows can widen another mesh's pad; pads only grow, as for a move -- the world
 * box and proxy record of every entry point, and the instance tree's boxes.  Picture, ray count and hit records are those of
 * art_upload_scene of the same scene with that mesh's vertices replaced, at the matrices in force, bit for bit.  Stream-ordered
 * exactly as art_refit_device and art_move_instances_device are: work enqueued before the call sees the old shape, work enqueued after
 * it the new one; the host waits only where the plan the call shares with art_move_instances_device is first built (the first of the
 * two calls after an upload).  Under art_init_devices every context is updated, the others from a peer copy of pos3f / nrm3f.  Refused
 * before anything is launched: no scene, a scene that is not instanced (art_refit_device moves a flat mesh), a scene committed through
 * gcore_commit_scene, mesh out of range, a mesh no instance shows, nverts other than that mesh's uploaded count, null pos3f, host memory
 * or another device's memory.  A vertex with a coordinate that is not finite or beyond 1e18 in magnitude is a bad vertex, counted as
 * art_refit_device counts them: the boxes holding it and every entry point with it among its records are empty (no ray enters them) and
 * the next art_synchronize fails with the count; a later good refit of the mesh or an upload clears that state.  The count is kept per
 * mesh: art_synchronize after a mesh refit reports the bad vertices of all meshes that still hold some, so a good refit of another mesh
 * does not hide them.  The placement test of art_move_instances_device runs again against the mesh's new box: an instance that the
 * grown mesh takes beyond 1e18 (coordinate times matrix) is emptied like a bad matrix's instance until a refit or a move brings it back
 * within reach, and nothing reports it -- the one case in which the picture is not the upload's.  After a large deformation
 * the trees cost more to walk than the ones a fresh art_upload_scene builds: art_get_mesh_tree_cost has the figure of the mesh's tree and
 * art_rebuild_mesh_tree_device builds it again. */
int  art_refit_mesh_device(int32_t mesh, const float* pos3f, const float* nrm3f, int64_t nverts, void* hip_stream);
/* refits = calls accepted, refit_ms = HIP events around device 0's kernels of the call, plan_ms = host time of building the plans (where
 * this call built them), bad_vertices = bad vertices counted on device 0 over all mesh refits, repads = meshes whose boxes a mesh refit
 * re-padded, over all mesh refits. */
typedef struct ArtMeshRefitInfo { uint64_t refits; double refit_ms; double plan_ms; uint64_t bad_vertices; uint64_t repads; } ArtMeshRefitInfo;
int  art_get_mesh_refit_info(ArtMeshRefitInfo* out);   /* cumulative since art_upload_scene; waits like art_get_move_info */

/* A new instance tree for an instanced scene whose instances have moved: the other half of
 * art_move_instances_device and art_refit_mesh_device, which keep the tree's topology.  The 4-wide tree over the entry points' world
 * boxes is built again on the GPU from the proxy records as they lie in HBM at the call -- the upload's tight boxes at the placement
 * of the last accepted move (or the upload's), mesh refits included -- by the GPU binned-SAH builder whatever "bvh_builder" says, with
 * the parameters art_upload_scene gives the instance tree (width 4, one entry point per leaf, default costs and pads), the proxies fed
 * in the upload's order (entry points by instance, then by where they enter the mesh's tree) and the nodes and records numbered as
 * the host builder numbers them.  The entry points stay as built: the inst_open choice, the instance table, where every entry point
 * enters its mesh and the numbering do not change, and nothing of the meshes is touched but the position of their quantised nodes --
 * the merged node array holds the instance tree first, so a tree of another node count moves them, and every inner entry word and
 * every entry point's node word moves with them.  With "inst_open" 1 the instance tree, its proxy records and its part of the node
 * array are the ones art_upload_scene at the matrices in force builds, byte for byte; picture, ray count and hit records do not change
 * in any case.  Ordering and failure as for art_rebuild_device: the call waits for what hip_stream (NULL: the library's stream) and the
 * library's streams hold, returns when the new tree is committed, and a failure leaves every context as it was; under
 * art_init_devices every context builds from its own proxy records before any context swaps.  A later move or mesh refit works
 * against the new tree.  Refused before anything is launched: no scene, a flat scene (art_rebuild_device builds that tree), a scene
 * committed through gcore_commit_scene, fewer than two entry points, and bad matrices or bad vertices in force (the message names the
 * count; a good move or refit clears it). */
int  art_rebuild_instance_tree_device(void* hip_stream);
/* Cumulative since art_upload_scene: gather_ms = HIP events around device 0's proxy gather, build_ms = HIP events around device 0's
 * builds, host_ms = host time inside the calls (all contexts, read-back, re-plan and commit included).  A failed call is not counted. */
typedef struct ArtInstanceRebuildInfo { uint64_t rebuilds; double gather_ms, build_ms, host_ms; } ArtInstanceRebuildInfo;
int  art_get_instance_rebuild_info(ArtInstanceRebuildInfo* out);   /* cumulative since art_upload_scene */
/* art_get_tree_cost's figure for the instance tree in HBM, from its binary32 packets: root_area = A(union of the root's used child
 * boxes), node_visits = 1 + sum over inner slots of A / root_area, leaf_visits = the expected number of entry points entered (sum over
 * leaf slots), tri_tests = the same weighted by the leaf's count (equal to leaf_visits: one entry point per leaf).  Empty slots and slots
 * a bad update emptied add nothing.  What a caller compares before and after art_rebuild_instance_tree_device; the library sets no
 * policy.  Fails without a scene, on a flat scene and on a scene committed through gcore_commit_scene. */
int  art_get_instance_tree_cost(ArtTreeCost* out);                 /* device 0; waits for the library's stream */

/* A new tree for one mesh of an instanced scene whose vertices have moved: the other half of
 * art_refit_mesh_device, which keeps the tree's topology, and the counterpart of art_rebuild_instance_tree_device.  The call takes no
 * vertices: mesh `mesh`'s 4-wide tree is built again on the GPU from that mesh's triangle records as they lie in HBM at the call --
 * after whatever art_refit_mesh_device has written -- by the GPU binned-SAH builder whatever "bvh_builder" says, with the parameters
 * art_upload_scene gives a mesh (width 4, default leaf size and costs, the scene's relative pad) and the absolute pad the mesh carries
 * at the call (pads only grow: the build's, or what a later move or refit widened it to), the corners fed in the order of the
 * triangles' indices in the mesh and the nodes and records numbered as the host builder numbers them.  Indices, material ids, shading
 * records, matrices, the other meshes' records, the entry points and the instance tree are not touched; the mesh's records are
 * reordered into the new leaves.  The meshes' trees lie one after the other, so a tree of another node count moves every mesh behind
 * it: their nodes, their inner entry words, their instances' node_base and every entry point's node word move with them.  After
 * art_refit_mesh_device + this call + art_rebuild_instance_tree_device the two-level scene is the one art_upload_scene of the deformed
 * scene builds with "inst_open" 1, word for word, where the pad is the upload's; picture, ray count and hit records do not change in any
 * case.  Ordering and failure as for art_rebuild_instance_tree_device: the call waits for what hip_stream (NULL: the library's stream)
 * and the library's streams hold, returns when the new tree is committed, and a failure (the allocator, the builder, a stack bound
 * above the trace kernels', the 31-bit node offsets, the check of the tree read back) leaves every context as it was; under
 * art_init_devices every context builds from its own records before any context swaps.  A later move, mesh refit, instance-tree rebuild
 * or mesh rebuild works against the new layout.  Refused before anything is launched: no scene, a flat scene (art_rebuild_device builds
 * that tree), a scene committed through gcore_commit_scene, mesh out of range, a mesh no instance shows, a mesh of fewer than two
 * triangles (art_refit_mesh_device moves it), bad matrices or bad vertices in force (the message names the counts; a good move or refit
 * clears them), and an instance of this mesh that the build opened ("inst_open": its entry points name subtrees of the old tree; opened
 * entry points of other meshes are relocated). */
int  art_rebuild_mesh_tree_device(int32_t mesh, void* hip_stream);
/* Cumulative since art_upload_scene: gather_ms = HIP events around device 0's record gather, build_ms = HIP events around device 0's
 * builds, host_ms = host time inside the calls (all contexts, read-back, renumbering and commit included).  A failed call is not counted. */
typedef struct ArtMeshRebuildInfo { uint64_t rebuilds; double gather_ms, build_ms, host_ms; } ArtMeshRebuildInfo;
int  art_get_mesh_rebuild_info(ArtMeshRebuildInfo* out);   /* cumulative since art_upload_scene; a failed call is not counted */
/* art_get_tree_cost's figure for the tree of mesh `mesh` of an instanced scene as it lies in HBM, in object space, from its binary32
 * packets.  Empty slots and slots a bad refit emptied add nothing.  What a caller compares after art_refit_mesh_device to decide when to
 * call art_rebuild_mesh_tree_device; the library sets no policy.  Refused as art_rebuild_mesh_tree_device refuses, but for bad state in
 * force and opened instances, which do not concern the figure. */
int  art_get_mesh_tree_cost(int32_t mesh, ArtTreeCost* out);   /* device 0; waits for the library's stream */

int  art_export_bvh(float* nodes, int64_t node_floats_cap, float* tris, int64_t tri_floats_cap, ArtBvhInfo* info);

/* Diagnostic: the two-level tree of an instanced scene as it lies in device 0's HBM right now -- what the trace kernels read, after
 * whatever art_move_instances_device and art_refit_mesh_device have done to it (the host's copies of the build are stale from the first
 * update on).  The call waits for the library's stream (an update enqueued on another stream is ordered before it, as for art_export_bvh
 * after a refit), copies, launches nothing and changes nothing.  buf == NULL, or a NULL pointer in it: that array is not wanted (sizes
 * only); cap[k] is the capacity of the k-th pointer of ArtTwoLevelBuffers in 32-bit words, a buffer that is too small fails the call.
 *   inst        32 words per entry point: the DevInstance records (m, minv, node_base, tri_base, shade_base, root_entry, qroot, inst, 2 pad
 *               words); the first n_inst are the instances
 *   tlas_nodes  32 per node of the instance tree: its binary32 packets      tlas_tris   12 per entry point: the proxy records
 *   blas_nodes  32 per node of the meshes' trees, one mesh after the other  blas_tris   12 per triangle record of the meshes
 *   qnodes      16 per node: the merged quantised array, the instance tree's n_tlas_nodes first, then the meshes' n_blas_nodes
 *   mesh_pad    1 per mesh: the absolute pad its boxes carry                mesh_box    6 per mesh: the object-space box of its good records
 *   mesh_base   3 per mesh: first node in blas_nodes, first record in blas_tris (-1: no instance shows the mesh), first node in qnodes
 *   node_mesh   1 per node of blas_nodes: its mesh
 * Before the first update the per-mesh values are the build's, afterwards the ones the kernels maintain (`updated` = 1).  The info also
 * carries the rules an update applies: the meshes' relative pad and the floor of their absolute pad, the scene's extent without the
 * instances, and the instance tree's pad rule.  Refused: no scene, a scene committed through gcore_commit_scene, a flat scene
 * (art_export_bvh exports that tree). */
typedef struct ArtTwoLevelInfo {
  int32_t n_inst, n_entry, n_mesh, n_tlas_nodes, n_blas_nodes, n_records, inst_shift, updated;
  float   mesh_pad_rel, mesh_pad_min, scene_extent, tlas_pad_rel, tlas_pad_abs; int32_t reserved_;
} ArtTwoLevelInfo;
typedef struct ArtTwoLevelBuffers {
  uint32_t* inst; float* tlas_nodes; float* tlas_tris; float* blas_nodes; float* blas_tris; uint32_t* qnodes;
  float* mesh_pad; float* mesh_box; int32_t* mesh_base; int32_t* node_mesh;
  int64_t cap[10];
} ArtTwoLevelBuffers;
int  art_export_two_level(ArtTwoLevelInfo* info, const ArtTwoLevelBuffers* buf);
int  art_get_stats(ArtStats* out);
/* The wavefront stages around the trace kernel (device 0, cumulative since art_resize; cooperative schedule): GPU time per kind of
 * kernel (HIP events on the launch stream, like ArtStats::trace_ms) and the work items every bounce read and kept -- what bench.py's
 * `stages` object and its whole-job roofline are made of.  items_in[b] / items_out[b]: input items of bounce b (b = 0: the camera paths)
 * and the items it wrote for bounce b + 1. */
typedef struct ArtStageStats {
  double   shade_ms, raygen_ms, fold_ms;    /* k_shade_compact (all instantiations) | k_raygen | k_resolve_last + k_fold_level + k_accumulate */
  uint64_t shade_launches, batches;
  uint64_t items_in[16], items_out[16];
} ArtStageStats;
int  art_get_stage_stats(ArtStageStats* out);
/* Camera rays the render passes generated and TRACED (every device, cumulative since art_resize; a host-side count, nothing waits).
 * ArtStats::rays counts queries ANSWERED -- one camera query per sample, the reference's Find_Closest_Hit calls -- but a camera ray
 * depends on (pixel, sample & 3) alone, so with option "camera_dedup" [1] a batch of pn pixels x sn samples generates and traces only
 * its 4 x pn distinct rays (sn is a multiple of 4 with AA on; pn rays with AA off) and bounce 0 reads every sample's hit from its distinct ray: the same picture and
 * the same ArtStats.  With the option 0, with "count_tests" 1 and on the one-ray-per-lane schedule every sample's ray is traced. */
int  art_get_camera_rays_traced(uint64_t* out);
/* Tuning / test options (defaults in brackets):  "trace_kernel" [0] 0 cooperative, 1 one ray per lane;  "batch_paths" [128M];
 * "blocks_per_cu" [occupancy];  "count_tests" [0];  "camera_dedup" [1] (art_get_camera_rays_traced);  "camera_order" [1] 0 bounce 0 visits the path slots in slot order, 1 tile-major (same picture);  "node_min" [0 = 4, instanced scenes 2];  "refill_min" [2];  "ray_chunk" [48];  "queue_segments" [8];  "shadow_anyhit" [1];
 * "lds_stack_cap" [0 = automatic];  BVH build (take effect at the next art_upload_scene): "bvh_width" [4] lanes per ray = children
 * per node, 4 or 8;  "bvh_builder" [3] 3 binned SAH on the GPU (the tree of 0, built in milliseconds), 0 binned SAH on the host, 1 LBVH on the GPU, 2 PLOC on the GPU;  "bvh_ploc_radius" [8];  "bvh_spatial_splits" [0];  "bvh_max_leaf" [width];
 * "bvh_leaf_base_milli", "bvh_node_cost_milli", "bvh_tri_cost_milli".  The wavefront stages: "shade_per" [0 = measured; 2 | 4 items per thread],
 * "skip_null_shadow" [0] (1: a shadow ray whose explicit colour is exactly zero under either verdict -- the light sample behind the
 * surface, a BxDF that is zero there -- is neither traced nor counted: the same picture, but fewer rays in ArtStats than the reference issues, integrators.adb:270.
 * 0: the cooperative schedule still answers such a query without a tree walk and counts it; "count_tests" = 1 and "trace_kernel" = 1 walk every one).  Instanced scenes: "inst_coop" [1] the cooperative kernel crosses the instance boundary (0: one ray per lane, the cross-check);
 * "inst_open" [0] entry points per instance the instance tree ends at (1 whole instances, n > 1 about n subtrees of the mesh's tree per
 * instance, 0 chosen from how much the instances' boxes overlap; takes effect at the next art_upload_scene).  How the path state is mapped
 * (round 6, profiles/r6_bimodal: the shade stage's rate depends on the size of the pieces its 35-74 GB are mapped in; the picture never does):
 * "paths_spread" [-1] chunk size in MB -- the path state as one address range over separately created physical chunks (HIP virtual memory
 * management; falls back to hipMalloc); -1: 64 MB chunks for a path state of 1 GB or more, 0: plain hipMalloc (13-17 % slower stages in
 * about half of the processes).  The options "shade_split", "paths_spread_holes", "paths_contiguous" and "hot_pad" are removed.
 * Device queries: "query_slice" [2^24] rays per slice (112 bytes of scratch per ray of a slice; 1 .. 2^28).
 * Test options: "inject_lost" (the next pass counts one lost path: art_synchronize must fail), "spread_fail_at" (creating that chunk of the
 * path state fails: everything created so far is undone and the path state comes from hipMalloc), "lds_stack_cap". */
int  art_set_option(const char* name, int64_t value);
const char* art_last_error(void);
void art_shutdown(void);

/* ---- legacy geometry-core seam: embree_connect.cpp:51-244 / scene_hydra_embree.adb:37-66 -------- */

typedef struct HitCpp {          /* embree_connect.cpp:186-194, 36 bytes */
  int32_t primIndex;
  int32_t geomIndex;
  int32_t instIndex;
  float   t;
  float   normal[3];             /* unnormalised geometric normal Ng = cross(B-A, C-A) */
  float   texCoord[2];           /* barycentrics u, v */
} HitCpp;

void gcore_init_and_clear(void);                                                       /* :60-67  */
void gcore_destroy(void);                                                              /* :51-58  */
int  gcore_add_mesh_3f(const float* a_vertices3f, int a_vertexNum, const int* a_indices, int a_indicesNum);  /* :69-144: returns mesh id, copies the data */
void gcore_instance_meshes(int a_geomId, const float* a_matrices16f, int a_matrixNum); /* :147-184: 3x4 row-major taken from each 16-float block */
void gcore_commit_scene(void);                                                         /* :241-244: BVH build + upload */
#ifdef __cplusplus
bool gcore_closest_hit(const float a_rayPos[3], const float a_rayDir[3], float t_near, float t_far, HitCpp* pHit);  /* :196-238 */
#else
_Bool gcore_closest_hit(const float a_rayPos[3], const float a_rayDir[3], float t_near, float t_far, HitCpp* pHit);
#endif

/* Scene representation chosen by gcore_commit_scene: -1 automatic (one tree per mesh + a tree over the instances from 16 instances on,
 * like Embree's instance geometries, embree_connect.cpp:147-184; below that every instance is flattened into one world-space mesh),
 * 0 always flatten, 1 always two-level. */
void gcore_set_two_level(int mode);
/* Where a single-ray gcore_closest_hit is answered: 0 (default, round 4) on the calling thread -- a host walk of the committed tree, the
 * same tree, walk and triangle arithmetic as the GPU kernels, so the same hit bit for bit: what the reference's call pattern needs (28
 * tasks, one ray each: scene_hydra_embree.adb:426-446; Embree's rtcIntersect1 also runs on the caller's core, embree_connect.cpp:218);
 * 1: concurrent callers are combined into shared GPU launches (rounds 2-3; kept for A/B and for the host == GPU parity test). */
void gcore_set_single_ray_on_gpu(int on);
/* Batch form (extension; no counterpart in embree_connect.cpp): t_near / t_far may be NULL for 0 / 1e5; returns the number of hits. */
int  gcore_closest_hit_n(int a_rayNum, const float* a_rayPos3f, const float* a_rayDir3f, const float* t_near, const float* t_far,
                         HitCpp* pHits, unsigned char* pFound);

#ifdef __cplusplus
}
#endif
#endif
