// art_device_entries.cpp -- the entries of the C ABI (include/art_hip.h) that work on the caller's device memory in the caller's stream
// order: art_trace_rays_device and art_occluded_rays_device (art_query.hip), art_render_aovs_device and art_render_aovs_motion_device
// (art_aov.hip), art_aovs_rays_device and art_camera_rays_device (art_aov_rays.hip), the three a-trous filters (art_denoise.hip), art_temporal_device and art_temporal_motion_device (art_temporal.hip),
// art_adaptive_estimate_device (art_adaptive.hip), art_svgf_spatial_variance_device (art_svgf_spatial.hip), art_auto_exposure_device and
// art_display_device (art_display.hip), art_upsample_device (art_upsample.hip), art_temporal_upsample_device (art_temporal_upsample.hip), art_firefly_device (art_firefly.hip), art_bloom_device (art_bloom.hip); with them art_trace_rays, the
// host-pointer query the device ones are held to.  What they share is written once: the check of a list of the caller's planes
// (check_planes), growing a scratch while nothing uses it (grow_idle), and the ordered call (ordered_call, art_api_internal.h).  An entry
// is its own refusals, its plane list, its size arithmetic and its launches; art_render.cpp's mask compaction uses the same pieces.
// Invariants of every entry: every check comes before the first launch; leave() runs on every way out past enter(), so the context
// stream is ordered after the call also when a launch failed; no entry takes an event pair, so ArtStats and ArtStageStats do not see them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "art_api_internal.h"
#include "art_adaptive.h"
#include "art_bloom.h"
#include "art_denoise.h"
#include "art_display.h"
#include "art_firefly.h"
#include "art_motion.h"
#include "art_query.h"
#include "art_shade.h"      // surface_at: trace_rays finishes its hit records on the host
#include "art_svgf_spatial.h"
#include "art_temporal.h"
#include "art_temporal_upsample.h"
#include "art_upsample.h"

namespace art {

// ---- what the entries share ---------------------------------------------------------------------------------------------------------
// A caller's buffer must be device memory of this context's GPU, and (where HIP knows the allocation) hold `bytes` from `p` on.
static int check_device_ptr(const void* p, size_t bytes, const char* what) {
  Ctx& c = g_ctx;
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return fail(std::string(what) + " is not device memory (hipPointerGetAttributes failed)"); }
  if (at.type != hipMemoryTypeDevice) return fail(std::string(what) + " is not device memory (host or unregistered pointer)");
  if (at.device != c.device) return fail(std::string(what) + " is memory of device " + std::to_string(at.device) + ", the library runs on device " + std::to_string(c.device));
  hipDeviceptr_t base = nullptr; size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess) {
    if ((const char*)p + bytes > (const char*)base + size) return fail(std::string(what) + " is smaller than the query needs (" + std::to_string(bytes) + " bytes)");
  } else (void)hipGetLastError();       // (memory HIP cannot size, e.g. a virtual-memory mapping: the type and the device were checked)
  return 0;
}
int check_planes(std::initializer_list<DevPlane> planes) {
  for (const DevPlane& x : planes) if (x.p && check_device_ptr(x.p, x.bytes, x.what)) return 1;
  return 0;
}
int grow_idle(const StreamOrder& order, const GrowList& want) {
  bool grow = false;
  for (const Grow& w : want) grow = grow || (w.buf && w.buf->bytes < w.bytes);
  if (!grow) return 0;
  HIP_TRY(hipStreamSynchronize(order.cs));
  if (order.other()) HIP_TRY(hipStreamSynchronize(order.qs));
  for (const Grow& w : want) if (w.buf && ensure(*w.buf, w.bytes)) return 1;
  return 0;
}
int end_ordered(StreamOrder& order, const char* name, int rc) {
  if (hipGetLastError() != hipSuccess && !rc) rc = fail(std::string(name) + ": kernel launch failed");
  if (order.leave()) return 1;          // (also after a failed launch)
  return rc;
}

// The scratch of the queries and the AOV pass for slices of S rays: b_query = a counter sink (256 B) | 7 SoA floats and the shadow minimum
// per ray | the hit records; and what a trace launch over a slice needs of b_queue and b_ovf, which the render passes use as well.
struct QuerySlice {
  unsigned long long* sink; float *ox, *oy, *oz, *dx, *dy, *dz, *tf, *shm; DevHit* hit;
  static GrowList scratch(size_t S, bool coop) {
    Ctx& c = g_ctx;
    int entries; bool ovf; stack_plan(entries, ovf);
    return {Grow{&c.b_query, 256 + S * (8 * 4 + sizeof(DevHit))}, Grow{coop ? &c.b_queue : nullptr, (S + kRecSlack) * kTraceRecBytes},
            Grow{coop && ovf ? &c.b_ovf : nullptr, S * sizeof(int)}};
  }
  explicit QuerySlice(size_t S) {       // (after the scratch has grown)
    char* base = (char*)g_ctx.b_query.p;
    float* f = (float*)(base + 256);
    sink = (unsigned long long*)base;
    ox = f; oy = f + S; oz = f + 2 * S; dx = f + 3 * S; dy = f + 4 * S; dz = f + 5 * S; tf = f + 6 * S; shm = f + 7 * S;
    hit = (DevHit*)(f + 8 * S);         // 16-byte aligned: the sink and 32 S bytes precede it
  }
  // the slice's rays as the trace launch sees them.  shadow_minima: every ray is a shadow ray (shadow_begin = 0); else a closest-hit query
  DevPaths paths(bool shadow_minima) const {
    DevPaths q; std::memset(&q, 0, sizeof q);
    q.ray_ox = ox; q.ray_oy = oy; q.ray_oz = oz; q.ray_dx = dx; q.ray_dy = dy; q.ray_dz = dz; q.ray_tfar = tf; q.hit = hit;
    q.sh_min_t = shadow_minima ? shm : nullptr; q.P = 0;
    return q;
  }
  // untimed, and the rays are counted into the sink: ArtStats does not see them
  TraceLaunch launch(hipStream_t qs, int kernel) const { return {qs, kernel, /*count_tests=*/false, /*timed=*/false, nullptr, nullptr, /*live_rays=*/sink}; }
};

// ---- art_trace_rays: rays and hits in host memory, on the context stream; the call waits ------------------------------------------------
int trace_rays(const float* origins, const float* dirs, const float* tfar, int64_t n, ArtHit* out, int kernel, ArtStats* st) {
  Ctx& c = g_ctx;
  if (!c.scene_ready) return fail("no scene uploaded");
  if (n <= 0 || n > (1ll << 28) || !origins || !dirs || !out) return fail("art_trace_rays: bad arguments");
  if (kernel != TRACE_COOP && kernel != TRACE_SIMPLE) return fail("art_trace_rays: unknown kernel");
  const size_t N = (size_t)n;
  if (ensure(c.b_rays, N * 12 * 4)) return 1;      // 7 N ray floats, N of padding, N 16-byte hit records
  std::vector<float> soa(7 * N);
  for (size_t i = 0; i < N; ++i) {
    soa[i] = origins[3 * i]; soa[N + i] = origins[3 * i + 1]; soa[2 * N + i] = origins[3 * i + 2];
    soa[3 * N + i] = dirs[3 * i]; soa[4 * N + i] = dirs[3 * i + 1]; soa[5 * N + i] = dirs[3 * i + 2];
    soa[6 * N + i] = tfar ? tfar[i] : kInfinity;
  }
  float* d = (float*)c.b_rays.p;
  HIP_TRY(hipMemcpyAsync(d, soa.data(), 7 * N * 4, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemsetAsync(d + 8 * N, 0xff, 4 * N * 4, c.stream));
  if (st) HIP_TRY(hipMemsetAsync(c.d_counters + CNT_STATS, 0, 8 * sizeof(unsigned long long), c.stream));
  DevPaths q; std::memset(&q, 0, sizeof q);
  q.ray_ox = d; q.ray_oy = d + N; q.ray_oz = d + 2 * N; q.ray_dx = d + 3 * N; q.ray_dy = d + 4 * N; q.ray_dz = d + 5 * N; q.ray_tfar = d + 6 * N;
  q.hit = (DevHit*)(d + 8 * N);                                      // 16-byte aligned: the buffer is, and 8 N floats precede it
  const TraceLaunch launch = {c.stream, kernel, /*count_tests=*/st != nullptr, /*timed=*/st != nullptr};      // without stats: no events, no counter read-back (the per-ray seam)
  if (trace(q, (int)n, launch)) return 1;
  std::vector<DevHit> hits(N);
  HIP_TRY(hipMemcpyAsync(hits.data(), d + 8 * N, N * sizeof(DevHit), hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  HIP_TRY(hipGetLastError());
  HostScene& hs = c.host_scene;
  if (hs.m_shade_stale) {                                            // a refit rewrote the normals in HBM (the stream is idle: synchronised above)
    HIP_TRY(hipMemcpy(hs.m_shade.data(), c.b_m_shade.p, hs.m_shade.size() * sizeof(float), hipMemcpyDeviceToHost));
    hs.m_shade_stale = false;
  }
  if (hs.inst_stale) {                                               // a move rewrote the matrices in HBM
    HIP_TRY(hipMemcpy(hs.inst.data(), c.b_inst.p, hs.inst.size() * sizeof(DevInstance), hipMemcpyDeviceToHost));
    hs.inst_stale = false;
  }
  bind_host_pointers(hs);
  for (size_t i = 0; i < N; ++i) {
    ArtHit& h = out[i];
    const uint32_t key = hits[i].key;
    h.t = hits[i].t; h.u = hits[i].u; h.v = hits[i].v;
    if (key == KEY_MISS) { h.is_hit = 0; h.prim_type = -1; h.prim_index = -1; h.mat_id = -1; h.mat = -1; h.normal[0] = h.normal[1] = h.normal[2] = 0.0f; continue; }
    const f3 o = mk3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), dd = mk3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    const Surface sf = surface_at(hs.hdr, o, dd, h.t, key, h.u, h.v);
    const uint32_t cls = key & ~KEY_INDEX_MASK;
    h.is_hit = 1; h.prim_index = (int32_t)(key & KEY_INDEX_MASK); h.mat_id = sf.mat_id; h.mat = sf.mat;
    h.prim_type = (cls == KEY_CORNELL) ? 0 : (cls == KEY_SPHERE) ? 1 : (cls == KEY_QUAD) ? 3 : 2;
    h.normal[0] = sf.normal.x; h.normal[1] = sf.normal.y; h.normal[2] = sf.normal.z;
  }
  if (st) {
    if (synchronize()) return 1;
    *st = c.stats;
  }
  return 0;
}

// ---- device-resident ray queries (art_trace_rays_device / art_occluded_rays_device) ----------------------------------------------
// hits (closest hit) or occluded (occlusion): n rays in slices of query_slice, every launch on the stream `st` names.  On another
// stream the query waits for what the context stream holds, and the context stream waits for the query.
int query_rays(const float* o3, const float* d3, const float* tnear, const float* tfar, int64_t n, ArtHit* hits, uint8_t* occluded, int kernel, hipStream_t st) {
  Ctx& c = g_ctx;
  const char* name = hits ? "art_trace_rays_device" : "art_occluded_rays_device";
  if (ensure_device()) return 1;
  if (n < 0 || n > 0x7fffffffll) return fail(std::string(name) + ": n must be 0 .. 2^31 - 1");
  if (kernel != TRACE_COOP && kernel != TRACE_SIMPLE) return fail(std::string(name) + ": unknown kernel");
  if (n == 0) return 0;
  if (!c.scene_ready) return fail("no scene uploaded");
  if (!o3 || !d3 || (!hits && !occluded)) return fail(std::string(name) + ": null ray or output buffer");
  const size_t N = (size_t)n;
  if (check_planes({{o3, 12 * N, "origins"}, {d3, 12 * N, "dirs"}, {tnear, 4 * N, "tnear"}, {tfar, 4 * N, "tfar"}, {hits, sizeof(ArtHit) * N, "hits_out"},
                    {occluded, N, "occluded_out"}}))
    return 1;
  const size_t S = (size_t)std::min<int64_t>(n, c.opt.query_slice);
  return ordered_call(name, st, QuerySlice::scratch(S, kernel == TRACE_COOP), [&](hipStream_t qs) {
    const QuerySlice sl(S);
    const TraceLaunch launch = sl.launch(qs, kernel);
    for (size_t s0 = 0; s0 < N; s0 += S) {
      const int m = (int)std::min(S, N - s0);
      QueryArgs Q; std::memset(&Q, 0, sizeof Q);
      Q.n = m; Q.o3 = o3 + 3 * s0; Q.d3 = d3 + 3 * s0; Q.tnear = tnear ? tnear + s0 : nullptr; Q.tfar = tfar ? tfar + s0 : nullptr;
      Q.ox = sl.ox; Q.oy = sl.oy; Q.oz = sl.oz; Q.dx = sl.dx; Q.dy = sl.dy; Q.dz = sl.dz; Q.tf = sl.tf;
      Q.shm = occluded ? sl.shm : nullptr; Q.hit = sl.hit;
      Q.out = hits ? (uint32_t*)(hits + s0) : nullptr; Q.occluded = occluded ? occluded + s0 : nullptr;
      launch_query_pack(qs, Q);
      if (trace(sl.paths(/*shadow_minima=*/occluded != nullptr), m, launch)) return 1;
      if (hits) launch_query_finalize(qs, c.scene, Q);
      else launch_query_occluded(qs, Q);
    }
    return 0;
  });
}

// art_render_aovs_device: the whole frame's camera rays (k per pixel) in slices of whole pixels, k * pixels <= query_slice, through the
// queries' scratch and stream order; per slice k_aov_raygen, the render loop's trace launch, k_aov_resolve.
// motion3f (art_render_aovs_motion_device): the resolve's MOTION instantiation also writes the motion plane from src (art_motion.h); the
// flat mesh's index triples are the refit plan's, which is built here where no refit has (the one time the host waits).
int render_aovs(const ArtPassParams* p, const ArtAovBuffers* out, hipStream_t st, const ArtMotionSource* src, float* motion3f) {
  Ctx& c = g_ctx;
  const std::string name = motion3f ? "art_render_aovs_motion_device" : "art_render_aovs_device";
  static const ArtAovBuffers no_planes = ArtAovBuffers();
  if (!p) return fail(name + ": null ArtPassParams");
  if (!out && motion3f) out = &no_planes;
  if (!out) return fail(name + ": null ArtAovBuffers");
  if (!motion3f && !out->albedo3f && !out->normal3f && !out->depth && !out->alpha && !out->prim_type && !out->prim_index && !out->mat) return fail(name + ": no plane is wanted (all seven pointers are null)");
  if (motion3f && !src) return fail(name + ": motion3f needs an ArtMotionSource (null src)");
  if (!c.scene_ready) return fail(name + ": no scene uploaded");
  if (c.host_scene.gcore_seam) return fail(name + ": the scene was committed through gcore_commit_scene, which has no camera");
  if (c.width <= 0) return fail(name + ": no viewport (art_resize)");
  const int kernel = c.opt.trace_kernel;
  if (c.scene.n_inst > 0 && kernel != TRACE_COOP) return fail(name + ": an instanced scene is traced through the record schedule only (option trace_kernel = 0)");
  const bool instanced = c.scene.n_inst > 0;
  const bool flat_src = motion3f && (src->cur_pos3f || src->prev_pos3f), inst_src = motion3f && src->prev_m12f;
  if (motion3f) {
    if ((src->cur_pos3f != nullptr) != (src->prev_pos3f != nullptr)) return fail(name + ": cur_pos3f and prev_pos3f must both be given or both be null");
    if (flat_src && instanced) return fail(name + ": vertex arrays are given but the scene is instanced (its motion comes from prev_m12f)");
    if (inst_src && !instanced) return fail(name + ": prev_m12f is given but the scene is not instanced (its motion comes from cur_pos3f and prev_pos3f)");
    if (flat_src && c.host_scene.m_nverts == 0) return fail(name + ": vertex arrays are given but the scene has no ART_MESH_CLOSEST mesh");
    if (flat_src && src->nverts != c.host_scene.m_nverts) return fail(name + ": nverts " + std::to_string(src->nverts) + " differs from the uploaded mesh's " + std::to_string(c.host_scene.m_nverts));
    if (inst_src && src->n_instances != c.scene.n_inst) return fail(name + ": n_instances " + std::to_string(src->n_instances) + " differs from the uploaded count " + std::to_string(c.scene.n_inst));
  }
  if (ensure_device()) return 1;
  const int64_t npix = (int64_t)c.width * c.height;
  const size_t N = (size_t)npix;
  if (motion3f && check_planes({{motion3f, 12 * N, "motion3f"}, {src->cur_pos3f, 12 * (size_t)src->nverts, "cur_pos3f"}, {src->prev_pos3f, 12 * (size_t)src->nverts, "prev_pos3f"},
                                {src->prev_m12f, 48 * (size_t)src->n_instances, "prev_m12f"}}))      // (src is only read with the plane; the vertex arrays: both or neither)
    return 1;
  if (check_planes({{out->albedo3f, 12 * N, "albedo3f"}, {out->normal3f, 12 * N, "normal3f"}, {out->depth, 4 * N, "depth"}, {out->alpha, 4 * N, "alpha"},
                    {out->prim_type, 4 * N, "prim_type"}, {out->prim_index, 4 * N, "prim_index"}, {out->mat, 4 * N, "mat"}}))
    return 1;
  ArtPassParams pp = ArtPassParams();   // only aa_on and background are the caller's
  pp.aa_on = p->aa_on; std::memcpy(pp.background, p->background, 12);
  DevFrame F; make_frame(&pp, F);
  const int k = F.aa_on ? 4 : 1;
  const int64_t ns = std::min<int64_t>(npix, std::max<int64_t>(1, c.opt.query_slice / k));      // pixels per slice
  const size_t S = (size_t)(ns * k);                                                            // its rays: at most 2^28 (query_slice), or k
  if (grow_idle(StreamOrder(c, st), QuerySlice::scratch(S, kernel == TRACE_COOP))) return 1;      // (before the plan below, which may wait as well)
  mo::Source ms; std::memset(&ms, 0, sizeof ms);
  if (flat_src) {
    if (ensure_refit_plan()) return 1;
    ms.idx = (const int32_t*)c.refit.b_idx.p; ms.cur = src->cur_pos3f; ms.prev = src->prev_pos3f;
    if (!ms.idx) return fail(name + ": internal: the refit plan holds no index triples");
  }
  if (instanced && motion3f) { ms.inst = c.scene.inst; ms.prev_m = src->prev_m12f; ms.inst_shift = c.scene.inst_shift; }
  return ordered_call(name.c_str(), st, GrowList{}, [&](hipStream_t qs) {
    const QuerySlice sl(S);
    const TraceLaunch launch = sl.launch(qs, kernel);
    for (int64_t p0 = 0; p0 < npix; p0 += ns) {
      const int n = (int)std::min<int64_t>(ns, npix - p0);
      AovMotionArgs A; std::memset((void*)&A, 0, sizeof A);      // (its AovArgs part is all the launches without the plane see)
      A.motion = motion3f ? motion3f + 3 * p0 : nullptr; A.src = ms;
      A.n = n; A.k = k; A.pixel0 = (uint32_t)p0;
      A.ox = sl.ox; A.oy = sl.oy; A.oz = sl.oz; A.dx = sl.dx; A.dy = sl.dy; A.dz = sl.dz; A.tf = sl.tf; A.hit = sl.hit;
      A.albedo = out->albedo3f ? out->albedo3f + 3 * p0 : nullptr; A.normal = out->normal3f ? out->normal3f + 3 * p0 : nullptr;
      A.depth = out->depth ? out->depth + p0 : nullptr; A.alpha = out->alpha ? out->alpha + p0 : nullptr;
      A.prim_type = out->prim_type ? out->prim_type + p0 : nullptr; A.prim_index = out->prim_index ? out->prim_index + p0 : nullptr;
      A.mat = out->mat ? out->mat + p0 : nullptr;
      launch_aov_raygen(qs, F, c.scene, A);
      if (trace(sl.paths(/*shadow_minima=*/false), k * n, launch)) return 1;
      if (motion3f) launch_aov_resolve_motion(qs, F, c.scene, A);
      else launch_aov_resolve(qs, F, c.scene, A);
    }
    return 0;
  });
}

// art_aovs_rays_device: the caller's rays in slices of whole groups, k * groups <= query_slice (at least one group), through the queries'
// scratch and stream order; per slice k_aov_rays_pack, the render loop's trace launch, k_aov_rays_resolve.  No viewport is needed.
int aovs_rays(const ArtAovRaysParams* p, const float* o3, const float* d3, const float* tnear, const float* tfar, int64_t n, const ArtAovRayBuffers* out, hipStream_t st) {
  Ctx& c = g_ctx;
  const std::string name = "art_aovs_rays_device";
  if (!p) return fail(name + ": null ArtAovRaysParams");
  if (!out) return fail(name + ": null ArtAovRayBuffers");
  if (!out->albedo3f && !out->normal3f && !out->position3f && !out->depth && !out->alpha && !out->prim_type && !out->prim_index && !out->mat)
    return fail(name + ": no plane is wanted (all eight pointers are null)");
  if (p->group < 1 || p->group > 16) return fail(name + ": group must be 1..16");
  if (n < 0 || n > 0x7fffffffll) return fail(name + ": n_rays must be 0 .. 2^31 - 1");
  if (n % p->group != 0) return fail(name + ": n_rays " + std::to_string(n) + " is not a multiple of group " + std::to_string(p->group));
  if (n == 0) return 0;
  if (!o3 || !d3) return fail(name + ": null origins3f or dirs3f");
  if (!c.scene_ready) return fail(name + ": no scene uploaded");
  const int kernel = c.opt.trace_kernel;
  if (c.scene.n_inst > 0 && kernel != TRACE_COOP) return fail(name + ": an instanced scene is traced through the record schedule only (option trace_kernel = 0)");
  if (ensure_device()) return 1;
  const int k = p->group;
  const size_t N = (size_t)n, G = N / (size_t)k;
  if (check_planes({{o3, 12 * N, "origins3f"}, {d3, 12 * N, "dirs3f"}, {tnear, 4 * N, "tnear"}, {tfar, 4 * N, "tfar"}, {out->albedo3f, 12 * G, "albedo3f"},
                    {out->normal3f, 12 * G, "normal3f"}, {out->position3f, 12 * G, "position3f"}, {out->depth, 4 * G, "depth"}, {out->alpha, 4 * G, "alpha"},
                    {out->prim_type, 4 * G, "prim_type"}, {out->prim_index, 4 * G, "prim_index"}, {out->mat, 4 * G, "mat"}}))
    return 1;
  const size_t ns = std::min<size_t>(G, (size_t)std::max<int64_t>(1, c.opt.query_slice / k));     // groups per slice
  const size_t S = ns * (size_t)k;                                                                // its rays: at most 2^28 (query_slice), or k
  return ordered_call(name.c_str(), st, QuerySlice::scratch(S, kernel == TRACE_COOP), [&](hipStream_t qs) {
    const QuerySlice sl(S);
    const TraceLaunch launch = sl.launch(qs, kernel);
    for (size_t g0 = 0; g0 < G; g0 += ns) {
      const size_t r0 = g0 * (size_t)k;
      AovRaysArgs A; std::memset(&A, 0, sizeof A);
      A.n = (int)std::min(ns, G - g0); A.k = k;
      A.o3 = o3 + 3 * r0; A.d3 = d3 + 3 * r0; A.tnear = tnear ? tnear + r0 : nullptr; A.tfar = tfar ? tfar + r0 : nullptr;
      A.ox = sl.ox; A.oy = sl.oy; A.oz = sl.oz; A.dx = sl.dx; A.dy = sl.dy; A.dz = sl.dz; A.tf = sl.tf; A.hit = sl.hit;
      std::memcpy(A.background, p->background, 12);
      A.albedo = out->albedo3f ? out->albedo3f + 3 * g0 : nullptr; A.normal = out->normal3f ? out->normal3f + 3 * g0 : nullptr;
      A.position = out->position3f ? out->position3f + 3 * g0 : nullptr;
      A.depth = out->depth ? out->depth + g0 : nullptr; A.alpha = out->alpha ? out->alpha + g0 : nullptr;
      A.prim_type = out->prim_type ? out->prim_type + g0 : nullptr; A.prim_index = out->prim_index ? out->prim_index + g0 : nullptr;
      A.mat = out->mat ? out->mat + g0 : nullptr;
      launch_aov_rays_pack(qs, A);
      if (trace(sl.paths(/*shadow_minima=*/false), k * A.n, launch)) return 1;
      launch_aov_rays_resolve(qs, c.scene, A);
    }
    return 0;
  });
}

// art_camera_rays_device: one kernel into the caller's two arrays; no scratch.  It refuses where render_aovs refuses.
int camera_rays(const ArtPassParams* p, float* o3, float* d3, hipStream_t st) {
  Ctx& c = g_ctx;
  const std::string name = "art_camera_rays_device";
  if (!p) return fail(name + ": null ArtPassParams");
  if (!o3 || !d3) return fail(name + ": null origins3f or dirs3f");
  if (!c.scene_ready) return fail(name + ": no scene uploaded");
  if (c.host_scene.gcore_seam) return fail(name + ": the scene was committed through gcore_commit_scene, which has no camera");
  if (c.width <= 0) return fail(name + ": no viewport (art_resize)");
  if (ensure_device()) return 1;
  ArtPassParams pp = ArtPassParams();   // only aa_on is the caller's
  pp.aa_on = p->aa_on;
  DevFrame F; make_frame(&pp, F);
  const int64_t n = (int64_t)c.width * c.height * (F.aa_on ? 4 : 1);
  if (check_planes({{o3, 12 * (size_t)n, "origins3f"}, {d3, 12 * (size_t)n, "dirs3f"}})) return 1;
  return ordered_call(name.c_str(), st, GrowList{}, [&](hipStream_t qs) { launch_camera_rays(qs, F, c.scene, o3, d3, n); return 0; });
}

// ---- the image-space entries: they need no scene and no viewport --------------------------------------------------------------------
// The three a-trous filters of art_denoise.h over the caller's planes (A.P and the planes are set, dn::params_from_abi has passed), in a
// scratch of their own (b_denoise, shared: all run in the queries' stream order).  Scratch per pixel: two images, the guide records and
// the depth gradients, 56 bytes; the modes that carry a variance add the depth plane, 60 bytes.
static int run_denoise(const std::string& name, dn::Mode mode, DenoiseArgs& A, int iterations, hipStream_t st) {
  if (ensure_device()) return 1;
  Ctx& c = g_ctx;
  const bool v = dn::carries_variance(mode), plane = (mode == dn::Mode::SvgfVar);
  const size_t N = (size_t)A.P.W * (size_t)A.P.H;
  if (check_planes({{A.color, 12 * N, "color3f"}, {A.out, 12 * N, "out3f"}, {v ? A.moments : nullptr, (plane ? 4 : 8) * N, plane ? "variance1f" : "moments2f"},
                    {A.albedo, 12 * N, "albedo3f"}, {A.normal, 12 * N, "normal3f"}, {A.depth, 4 * N, "depth"}, {A.variance_out, 4 * N, "variance_out"}}))
    return 1;
  const size_t bytes = N * (3 * sizeof(dn::Rec4) + sizeof(dn::Rec2) + (v ? sizeof(float) : 0));
  return ordered_call(name.c_str(), st, GrowList{Grow{&c.b_denoise, bytes}}, [&](hipStream_t qs) {
    A.n = (int32_t)N;
    dn::Rec4* r4 = (dn::Rec4*)c.b_denoise.p;
    A.image[0] = r4; A.image[1] = r4 + N; A.guide = r4 + 2 * N; A.grad = (dn::Rec2*)(r4 + 3 * N); A.z = v ? (float*)(A.grad + N) : nullptr;
    launch_denoise(qs, mode, A, iterations);
    return 0;
  });
}

int denoise_device(const ArtDenoiseParams* p, const float* color3f, const float* albedo3f, const float* normal3f, const float* depth, float* out3f, hipStream_t st) {
  const std::string name = "art_denoise_device";
  DenoiseArgs A; std::memset(&A, 0, sizeof A);
  if (const char* why = dn::params_from_abi(p, color3f, albedo3f, normal3f, depth, out3f, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  A.color = color3f; A.albedo = albedo3f; A.normal = normal3f; A.depth = depth; A.out = out3f;
  return run_denoise(name, dn::Mode::Plain, A, p->iterations, st);      // (variant: one kernel exists, every tap from global memory; 0, 1 and 2 all select it)
}

// variance_plane: art_denoise_svgf_var_device, whose moments2f is the variance plane
int denoise_svgf_device(const ArtSvgfParams* p, const float* color3f, const float* moments2f, const float* albedo3f, const float* normal3f, const float* depth,
                        float* out3f, float* variance_out, hipStream_t st, bool variance_plane) {
  const std::string name = variance_plane ? "art_denoise_svgf_var_device" : "art_denoise_svgf_device";
  DenoiseArgs A; std::memset(&A, 0, sizeof A);
  if (const char* why = dn::params_from_abi(p, color3f, moments2f, albedo3f, normal3f, depth, out3f, variance_plane, A.P)) return fail(name + ": " + why);
  A.n_colours = p->n_colours;
  A.color = color3f; A.moments = moments2f; A.albedo = albedo3f; A.normal = normal3f; A.depth = depth; A.out = out3f; A.variance_out = variance_out;
  return run_denoise(name, variance_plane ? dn::Mode::SvgfVar : dn::Mode::Svgf, A, p->iterations, st);
}

// art_temporal_device: one kernel over the caller's planes and histories (art_temporal.h).  It has no scratch, so nothing can make the
// host wait.
int temporal_device(const ArtTemporalParams* p, const float* color3f, const float* moments2f, const float* normal3f, const float* depth, const int32_t* id,
                    const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out, hipStream_t st, const float* motion3f, const char* call) {
  const std::string name = call;
  TemporalArgs A; std::memset(&A, 0, sizeof A);
  if (const char* why = tp::params_from_abi(p, color3f, moments2f, normal3f, depth, id, hist_in, hist_out, A.P, motion3f)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  const size_t N = (size_t)A.P.cur.W * (size_t)A.P.cur.H, NP = (size_t)A.P.prev.W * (size_t)A.P.prev.H;
  if (check_planes({{color3f, 12 * N, "color3f"}, {moments2f, 8 * N, "moments2f"}, {hist_out, 48 * N, "hist_out"}, {hist_in, 48 * NP, "hist_in"},
                    {normal3f, 12 * N, "normal3f"}, {depth, 4 * N, "depth"}, {id, 4 * N, "id"}, {out3f, 12 * N, "out3f"}, {variance_out, 4 * N, "variance_out"},
                    {length_out, 4 * N, "length_out"}, {motion3f, 12 * N, "motion3f"}}))
    return 1;
  A.motion = motion3f; A.has_motion = motion3f ? 1 : 0;
  A.n = (int32_t)N; A.color = color3f; A.moments = moments2f; A.normal = normal3f; A.depth = depth; A.id = id;
  A.hist_in = (const tp::Rec4*)hist_in; A.hist_out = (tp::Rec4*)hist_out; A.out = out3f; A.variance_out = variance_out; A.length_out = length_out;
  return ordered_call(name.c_str(), st, GrowList{}, [&](hipStream_t qs) { launch_temporal(qs, A); return 0; });
}

// art_adaptive_estimate_device: one kernel over the caller's planes (art_adaptive.h); no scratch.
int adaptive_estimate_device(const ArtAdaptiveParams* p, const float* accum3f, const float* moments2f, const uint32_t* counts1u, float* mean3f, float* variance1f,
                             float* error1f, uint8_t* mask1b, hipStream_t st) {
  const std::string name = "art_adaptive_estimate_device";
  AdaptiveArgs A; std::memset(&A, 0, sizeof A);
  if (const char* why = ad::params_from_abi(p, accum3f, moments2f, counts1u, mean3f, variance1f, error1f, mask1b, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  const size_t N = (size_t)A.P.n;
  if (check_planes({{accum3f, 12 * N, "accum3f"}, {moments2f, 8 * N, "moments2f"}, {counts1u, 4 * N, "counts1u"}, {mean3f, 12 * N, "mean3f"},
                    {variance1f, 4 * N, "variance1f"}, {error1f, 4 * N, "error1f"}, {mask1b, N, "mask1b"}}))
    return 1;
  A.accum = accum3f; A.moments = moments2f; A.counts = counts1u; A.mean = mean3f; A.variance = variance1f; A.error = error1f; A.mask = mask1b;
  return ordered_call(name.c_str(), st, GrowList{}, [&](hipStream_t qs) { launch_adaptive_estimate(qs, A); return 0; });
}

// art_svgf_spatial_variance_device: one kernel over the caller's history and variance planes (art_svgf_spatial.h); no scratch.
int svgf_spatial_variance_device(const ArtSvgfSpatialParams* p, const void* hist, const float* variance_in1f, float* variance_out1f, hipStream_t st) {
  const std::string name = "art_svgf_spatial_variance_device";
  SvgfSpatialArgs A; std::memset(&A, 0, sizeof A);
  if (const char* why = sv::params_from_abi(p, hist, variance_in1f, variance_out1f, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  const size_t N = (size_t)A.P.W * (size_t)A.P.H;
  if (check_planes({{hist, 48 * N, "hist"}, {variance_in1f, 4 * N, "variance_in1f"}, {variance_out1f, 4 * N, "variance_out1f"}})) return 1;
  A.tiles_x = svgf_spatial_tiles_x(A.P.W);
  A.hist = (const sv::Rec4*)hist; A.variance_in = variance_in1f; A.variance_out = variance_out1f;
  return ordered_call(name.c_str(), st, GrowList{}, [&](hipStream_t qs) { launch_svgf_spatial(qs, A); return 0; });
}

// art_auto_exposure_device: the state's histogram is zeroed on the stream, then two kernels over the caller's plane and state
// (art_display.h); no scratch.
int auto_exposure_device(const ArtExposureParams* p, const float* color3f, void* state, hipStream_t st) {
  const std::string name = "art_auto_exposure_device";
  ExposureArgs A; std::memset(&A, 0, sizeof A);
  if (const char* why = dp::params_from_abi(p, color3f, state, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  const size_t N = (size_t)A.P.W * (size_t)A.P.H;
  if (check_planes({{color3f, 12 * N, "color3f"}, {state, 4 * (size_t)dp::kStateWords, "state"}})) return 1;
  A.n = (int32_t)N; A.color = color3f; A.state = (uint32_t*)state;
  return ordered_call(name.c_str(), st, GrowList{}, [&](hipStream_t qs) {
    HIP_TRY(hipMemsetAsync(A.state + 4, 0, 4 * (size_t)dp::kBins, qs));
    launch_auto_exposure(qs, A);
    return 0;
  });
}

// art_display_device: one kernel over the caller's planes (art_display.h); no scratch.
int display_device(const ArtDisplayParams* p, const float* color3f, const void* exposure_state, uint32_t* screen1u, float* ldr3f, hipStream_t st) {
  const std::string name = "art_display_device";
  DisplayArgs A; std::memset(&A, 0, sizeof A);
  if (const char* why = dp::params_from_abi(p, color3f, exposure_state, screen1u, ldr3f, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  const size_t N = (size_t)A.P.W * (size_t)A.P.H;
  if (check_planes({{color3f, 12 * N, "color3f"}, {exposure_state, 4 * (size_t)dp::kStateWords, "exposure_state"}, {screen1u, 4 * N, "screen1u"}, {ldr3f, 12 * N, "ldr3f"}}))
    return 1;
  A.color = color3f; A.state = (const uint32_t*)exposure_state; A.screen = screen1u; A.ldr = ldr3f;
  return ordered_call(name.c_str(), st, GrowList{}, [&](hipStream_t qs) { launch_display(qs, A); return 0; });
}

// art_upsample_device: the pack kernel over the lo frame into the denoisers' scratch (b_denoise: two records per lo pixel), then one
// kernel over the hi frame (art_upsample.h).
int upsample_device(const ArtUpsampleParams* p, const float* lo_color3f, const ArtUpsampleGuides* lo, const ArtUpsampleGuides* hi, float* out3f, uint8_t* fallback1b, hipStream_t st) {
  const std::string name = "art_upsample_device";
  UpsampleArgs A; std::memset((void*)&A, 0, sizeof A);
  if (const char* why = us::params_from_abi(p, lo_color3f, lo, hi, out3f, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  Ctx& c = g_ctx;
  const size_t N = (size_t)A.P.W * (size_t)A.P.H, NL = (size_t)A.P.LW * (size_t)A.P.LH;
  if (check_planes({{lo_color3f, 12 * NL, "lo_color3f"}, {lo->albedo3f, 12 * NL, "lo albedo3f"}, {lo->normal3f, 12 * NL, "lo normal3f"}, {lo->depth, 4 * NL, "lo depth"},
                    {lo->id, 4 * NL, "lo id"}, {hi->albedo3f, 12 * N, "hi albedo3f"}, {hi->normal3f, 12 * N, "hi normal3f"}, {hi->depth, 4 * N, "hi depth"},
                    {hi->id, 4 * N, "hi id"}, {out3f, 12 * N, "out3f"}, {fallback1b, N, "fallback1b"}}))
    return 1;
  if (const char* why = us::overlap_refusal(A.P, lo_color3f, lo, hi, out3f, fallback1b)) return fail(name + ": " + why);
  A.lo_color = lo_color3f; A.lo_albedo = lo->albedo3f; A.lo_normal = lo->normal3f; A.lo_depth = lo->depth; A.lo_id = lo->id;
  A.hi = us::HiGuides{hi->albedo3f, hi->normal3f, hi->depth, hi->id};
  A.out = out3f; A.fallback = fallback1b;
  return ordered_call(name.c_str(), st, GrowList{Grow{&c.b_denoise, 2 * NL * sizeof(us::Rec4)}}, [&](hipStream_t qs) {
    A.lo_c = (us::Rec4*)c.b_denoise.p; A.lo_g = A.lo_c + NL;
    launch_upsample(qs, A);
    return 0;
  });
}

// art_temporal_upsample_device: the pack kernel over the lo frame into the denoisers' scratch (b_denoise: three records per lo pixel),
// then one kernel over the hi frame and the two histories (art_temporal_upsample.h).
int temporal_upsample_device(const ArtTemporalUpsampleParams* p, const float* lo_color3f, const float* lo_moments2f, const ArtTemporalUpsampleGuides* lo,
                             const ArtTemporalUpsampleGuides* hi, const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out,
                             uint8_t* fallback1b, hipStream_t st) {
  const std::string name = "art_temporal_upsample_device";
  TemporalUpsampleArgs A; std::memset((void*)&A, 0, sizeof A);
  if (const char* why = tu::params_from_abi(p, lo_color3f, lo_moments2f, lo, hi, hist_in, hist_out, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  Ctx& c = g_ctx;
  const size_t N = (size_t)A.P.T.cur.W * (size_t)A.P.T.cur.H, NP = (size_t)A.P.T.prev.W * (size_t)A.P.T.prev.H, NL = (size_t)A.P.LW * (size_t)A.P.LH;
  if (check_planes({{lo_color3f, 12 * NL, "lo_color3f"}, {lo_moments2f, 8 * NL, "lo_moments2f"}, {lo->normal3f, 12 * NL, "lo normal3f"}, {lo->depth, 4 * NL, "lo depth"},
                    {lo->id, 4 * NL, "lo id"}, {hi->normal3f, 12 * N, "hi normal3f"}, {hi->depth, 4 * N, "hi depth"}, {hi->id, 4 * N, "hi id"},
                    {hi->motion3f, 12 * N, "hi motion3f"}, {hist_in, 48 * NP, "hist_in"}, {hist_out, 48 * N, "hist_out"}, {out3f, 12 * N, "out3f"},
                    {variance_out, 4 * N, "variance_out"}, {length_out, 4 * N, "length_out"}, {fallback1b, N, "fallback1b"}}))
    return 1;
  if (const char* why = tu::overlap_refusal(A.P, lo_color3f, lo_moments2f, lo, hi, hist_in, hist_out, out3f, variance_out, length_out, fallback1b)) return fail(name + ": " + why);
  A.lo_color = lo_color3f; A.lo_moments = lo_moments2f; A.lo_normal = lo->normal3f; A.lo_depth = lo->depth; A.lo_id = lo->id;
  A.normal = hi->normal3f; A.depth = hi->depth; A.id = hi->id; A.motion = hi->motion3f;
  A.hist_in = (const tu::Rec4*)hist_in; A.hist_out = (tu::Rec4*)hist_out;
  A.out = out3f; A.variance_out = variance_out; A.length_out = length_out; A.fallback = fallback1b;
  return ordered_call(name.c_str(), st, GrowList{Grow{&c.b_denoise, 3 * NL * sizeof(tu::Rec4)}}, [&](hipStream_t qs) {
    A.lo_a = (tu::Rec4*)c.b_denoise.p; A.lo_b = A.lo_a + NL; A.lo_c = A.lo_b + NL;
    launch_temporal_upsample(qs, A);
    return 0;
  });
}

// art_firefly_device: the key kernel over the frame into the denoisers' scratch (b_denoise: one float per pixel), then the window kernel
// over 16 x 16 tiles (art_firefly.h).
int firefly_device(const ArtFireflyParams* p, const float* color3f, const float* moments2f, const int32_t* id, float* out3f, float* moments_out2f, uint8_t* clamped1b, hipStream_t st) {
  const std::string name = "art_firefly_device";
  FireflyArgs A; std::memset((void*)&A, 0, sizeof A);
  if (const char* why = fi::params_from_abi(p, color3f, moments2f, out3f, moments_out2f, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  Ctx& c = g_ctx;
  const size_t N = (size_t)A.P.W * (size_t)A.P.H;
  if (check_planes({{color3f, 12 * N, "color3f"}, {moments2f, 8 * N, "moments2f"}, {id, 4 * N, "id"}, {out3f, 12 * N, "out3f"}, {moments_out2f, 8 * N, "moments_out2f"},
                    {clamped1b, N, "clamped1b"}}))
    return 1;
  if (const char* why = fi::overlap_refusal(A.P, color3f, moments2f, id, out3f, moments_out2f, clamped1b)) return fail(name + ": " + why);
  A.color = color3f; A.moments = moments2f; A.id = id; A.out = out3f; A.moments_out = moments_out2f; A.clamped = clamped1b;
  return ordered_call(name.c_str(), st, GrowList{Grow{&c.b_denoise, N * sizeof(float)}}, [&](hipStream_t qs) {
    A.keys = (float*)c.b_denoise.p;
    launch_firefly(qs, A);
    return 0;
  });
}

// art_bloom_device: the pyramid in the denoisers' scratch (b_denoise: one 16-byte record per texel of levels 1 .. M), the downsamples,
// the tail or the per-level blends, the mix (art_bloom.h).
int bloom_device(const ArtBloomParams* p, const float* color3f, const void* exposure_state, float* out3f, float* bloom3f, hipStream_t st) {
  const std::string name = "art_bloom_device";
  BloomArgs A; std::memset((void*)&A, 0, sizeof A);
  if (const char* why = bl::params_from_abi(p, color3f, exposure_state, out3f, bloom3f, A.P)) return fail(name + ": " + why);      // (before the device is looked for)
  if (ensure_device()) return 1;
  Ctx& c = g_ctx;
  const size_t N = (size_t)A.P.W * (size_t)A.P.H;
  if (check_planes({{color3f, 12 * N, "color3f"}, {exposure_state, bl::kStateBytes, "exposure_state"}, {out3f, 12 * N, "out3f"}, {bloom3f, 12 * N, "bloom3f"}})) return 1;
  A.color = color3f; A.state = (const uint32_t*)exposure_state; A.out = out3f; A.bloom = bloom3f;
  return ordered_call(name.c_str(), st, GrowList{Grow{&c.b_denoise, (size_t)A.P.off[A.P.made + 1] * sizeof(bl::Rec4)}}, [&](hipStream_t qs) {
    A.pyr = (bl::Rec4*)c.b_denoise.p;
    launch_bloom(qs, A);
    return 0;
  });
}

}  // namespace art
