// art_api.cpp -- C-ABI driver of the render backend (include/art_hip.h).  Owns the HBM-resident scene,
// the wavefront path buffers and the per-pass kernel schedule that replaces Ray_Tracer.Render_Pass'
// task pool (ray_tracer.adb:240-293):
//
//   per batch of P = pixels x samples path slots:
//     raygen -> [ trace(ext + shadow rays) -> shade(bounce) ] x max_depth -> trace(last shadow rays)
//            -> finish (inside-out radiance fold) -> accumulate (reference summation order)
//   then resolve (gamma, clamp, pack) when the caller asks for the LDR image.
//
// The path state, the trace launch and that schedule itself: art_render.cpp (batch shape and shade trial: art_pass_plan.h).
// The entries that work on the caller's device memory in the caller's stream order (ray queries, AOVs, denoisers, temporal, adaptive estimate): art_device_entries.cpp.
// The device-side scene updates (art_refit_device, art_rebuild_device, art_move_instances_device, art_refit_mesh_device, art_rebuild_instance_tree_device, art_get_tree_cost): art_update.cpp.
// There is no CPU fallback: every entry point that needs the GPU fails with art_last_error() set when
// HIP reports no usable device.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "art_api_internal.h"
#include "art_frame.h"
#include "art_lbvh.h"

namespace art {

Ctx g_devs[kMaxDevices];
int g_ndev = 1;
Ctx* g_cur = &g_devs[0];
std::mutex g_mu;
static ncclComm_t g_comms[kMaxDevices];
static bool g_comms_ready = false;     // distinct GPUs: the framebuffer reduce goes through RCCL
// events around every reduce on device 0's stream (art_get_reduce_info: the reduce's GPU time is part of the evidence of a multi-GPU run)
static EventPairs g_reduce_pairs;     // (a host that downloads every frame re-uses one pair)
static double g_reduce_ms = 0.0; static int g_reduces = 0, g_reduce_path = 0;
bool g_multi_api = false;              // the process came up through art_init_devices: passes carry host-clock marks (art_get_reduce_info), also with n = 1
static int g_passes = 0, g_passes_overlapped = 0;  // multi-device passes folded so far / those in which every device had started before any had finished
static void reset_reduce_info() {
  g_reduce_pairs.release(); g_reduce_ms = 0.0; g_reduces = 0; g_reduce_path = 0;
  g_passes = g_passes_overlapped = 0;
}
// completed pairs -> g_reduce_ms (device 0 current, its stream idle)
static void fold_reduce_events() { (void)g_reduce_pairs.fold(/*wait=*/true, [](float ms, uint8_t) { g_reduce_ms += ms; }); }
// multi-device mode: the host clock at which a device's stream reaches a point (hipLaunchHostFunc), so that the devices' pass times share
// ONE clock -- HIP events of different devices cannot be compared
static double host_ms() {
  static const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
void clock_cb(void* p) { *(double*)p = host_ms(); }
// every device's passes (all idle) -> busy / idle / start skew per device.  Pass i of every device is one Render_Pass: idle = the slowest
// device's end - this device's end (what an uneven tile deal costs), start skew = this device's start - the first device's start (what a
// host that enqueues device after device costs), overlapped = every device had started before any had finished.
static void fold_pass_clocks() {
  size_t n = SIZE_MAX;
  for (int k = 0; k < g_ndev; ++k) n = std::min(n, g_devs[k].pass_clock.size());
  if (!g_multi_api || n == SIZE_MAX) n = 0;
  for (size_t i = 0; i < n; ++i) {
    double first = 1e300, last_start = -1e300, first_end = 1e300, last = -1e300;
    for (int k = 0; k < g_ndev; ++k) { const Ctx::PassClock& pc = *g_devs[k].pass_clock[i]; first = std::min(first, pc.t0); last_start = std::max(last_start, pc.t0); first_end = std::min(first_end, pc.t1); last = std::max(last, pc.t1); }
    for (int k = 0; k < g_ndev; ++k) { Ctx& c = g_devs[k]; const Ctx::PassClock& pc = *c.pass_clock[i]; c.busy_ms += pc.t1 - pc.t0; c.idle_ms += last - pc.t1; c.start_skew_ms += pc.t0 - first; }
    g_passes += 1; if (last_start < first_end) g_passes_overlapped += 1;
  }
  for (int k = 0; k < g_ndev; ++k) { for (Ctx::PassClock* pc : g_devs[k].pass_clock) delete pc; g_devs[k].pass_clock.clear(); }
}
static bool g_same_gpu = false;        // rehearsal: several contexts on ONE physical GPU, the reduce is a local sum (no collective possible)
const bool g_debug_addr = getenv("ART_DEBUG_ADDR") != nullptr;   // development aid: device addresses of the path state per batch layout on stderr (profiles/r6_bimodal)
static thread_local std::string t_err;
static std::string g_err;

int fail(const std::string& msg) { g_err = msg; return 1; }

// make device k's context the current one (g_ctx) and its GPU the current HIP device
int use_dev(int k) {
  g_cur = &g_devs[k];
  if (g_cur->device >= 0) HIP_TRY(hipSetDevice(g_cur->device));
  return 0;
}
int ensure(DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return 0;
  b.release();
  HIP_TRY(hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return 0;
}

void DevBuf::release() {
  if (reserved) {                                        // a mapped range (alloc_spread)
    for (size_t i = 0; i < chunks.size(); ++i) { (void)hipMemUnmap((char*)p + i * chunk_bytes, chunk_bytes); (void)hipMemRelease(chunks[i]); }
    (void)hipMemAddressFree(p, reserved);
    chunks.clear(); reserved = 0; chunk_bytes = 0;
  } else if (p) (void)hipFree(p);
  p = nullptr; bytes = 0;
}

// `bytes` of device memory as ONE address range over separately created physical chunks of `chunk` bytes (Options::paths_spread_mb: the driver
// then maps the range in pieces no larger than a chunk, which is what the shade stage's forty streams want).  Every failure undoes what
// was done and reports it; the caller falls back to hipMalloc.
hipError_t alloc_spread(DevBuf& b, size_t bytes, size_t chunk, int device, int fail_at) {      // fail_at: test option spread_fail_at -- chunk number whose creation is made to fail
  hipMemAllocationProp prop; std::memset(&prop, 0, sizeof prop);
  prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = device;
  size_t gran = 0;
  hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
  if (e != hipSuccess || gran == 0) return e != hipSuccess ? e : hipErrorNotSupported;
  chunk = (chunk + gran - 1) / gran * gran;
  const size_t n = (bytes + chunk - 1) / chunk;
  void* va = nullptr;
  e = hipMemAddressReserve(&va, n * chunk, 0, nullptr, 0);
  if (e != hipSuccess) return e;
  std::vector<hipMemGenericAllocationHandle_t> got;
  size_t mapped = 0;
  auto undo = [&]() {
    for (size_t i = 0; i < mapped; ++i) (void)hipMemUnmap((char*)va + i * chunk, chunk);
    for (auto h : got) (void)hipMemRelease(h);
    (void)hipMemAddressFree(va, n * chunk);
    (void)hipGetLastError();
  };
  for (size_t i = 0; i < n; ++i) {
    hipMemGenericAllocationHandle_t h;
    e = ((int64_t)i == (int64_t)fail_at) ? hipErrorOutOfMemory : hipMemCreate(&h, chunk, &prop, 0);
    if (e != hipSuccess) { undo(); return e; }
    got.push_back(h);
  }
  for (size_t i = 0; i < n; ++i) {
    e = hipMemMap((char*)va + i * chunk, chunk, 0, got[i], 0);
    if (e != hipSuccess) { undo(); return e; }
    mapped = i + 1;
  }
  hipMemAccessDesc acc; std::memset(&acc, 0, sizeof acc);
  acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
  e = hipMemSetAccess(va, n * chunk, &acc, 1);
  if (e != hipSuccess) { undo(); return e; }
  b.p = va; b.bytes = bytes; b.chunks = std::move(got); b.chunk_bytes = chunk; b.reserved = n * chunk;
  return hipSuccess;
}

int ensure_device() {
  Ctx& c = g_ctx;
  if (c.device_ready) return 0;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail("no HIP device available (this library has no CPU path): " + std::string(hipGetErrorString(e)));
  if (c.device >= 0) HIP_TRY(hipSetDevice(c.device));
  HIP_TRY(hipGetDevice(&c.device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, c.device));
  c.num_cus = prop.multiProcessorCount;
  c.arch = prop.gcnArchName;
  // LDS per CU: 160 KB on gfx950 (MI355X_MICROARCH.md); the runtime's own figure where it is larger than the per-workgroup 64 KB
  c.lds_per_cu = (c.arch.rfind("gfx950", 0) == 0) ? 160 * 1024 : std::max<int>(64 * 1024, (int)prop.maxSharedMemoryPerMultiProcessor);
  HIP_TRY(hipMalloc(&c.d_cursor, kCursorInts * sizeof(int)));   // [0] work cursor, [1] live-ray queue length, [2] overflow queue length, [32*k] cursor of queue segment k
  HIP_TRY(hipMalloc(&c.d_counters, kCounters * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(c.d_counters, 0, kCounters * sizeof(unsigned long long)));
  c.device_ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------
static int upload_scene_arrays(HostScene& hs) {
  Ctx& c = g_ctx;
  if (upload(c.b_spheres, hs.spheres) || upload(c.b_sphere_mat, hs.sphere_mat) || upload(c.b_lights, hs.lights) ||
      upload(c.b_materials, hs.materials) || upload(c.b_bf_pos, hs.bf_pos) || upload(c.b_bf_nrm, hs.bf_nrm) ||
      upload(c.b_bf_uv, hs.bf_uv) || upload(c.b_bf_idx, hs.bf_idx) || (!hs.gpu_built && upload(c.b_nodes, hs.bvh.nodes)) || (!hs.gpu_built && upload(c.b_qnodes, hs.bvh.qnodes)) ||
      (!hs.gpu_built && upload(c.b_tris, hs.bvh.tris)) || upload(c.b_m_shade, hs.m_shade))
    return 1;
  if (hs.hdr.n_inst > 0 && (upload(c.b_inst, hs.inst) || upload(c.b_qnodes, hs.two.qnodes) || upload(c.b_tlas_nodes, hs.two.tlas.nodes) || upload(c.b_tlas_tris, hs.two.tlas.tris) ||
                            upload(c.b_blas_nodes, hs.two.blas_nodes) || upload(c.b_blas_tris, hs.two.blas_tris)))
    return 1;
  DevScene& s = c.scene;
  s = hs.hdr;
  if (hs.hdr.n_inst > 0) {
    s.inst = (const DevInstance*)c.b_inst.p; s.tlas_nodes = (const float*)c.b_tlas_nodes.p; s.tlas_tris = (const float*)c.b_tlas_tris.p;
    s.blas_nodes = (const float*)c.b_blas_nodes.p; s.blas_tris = (const float*)c.b_blas_tris.p;
  }
  s.spheres = (const DevSphere*)c.b_spheres.p; s.sphere_mat = (const int32_t*)c.b_sphere_mat.p;
  s.lights = (const DevLight*)c.b_lights.p; s.materials = (const DevMaterial*)c.b_materials.p;
  s.bf_pos = (const float*)c.b_bf_pos.p; s.bf_nrm = (const float*)c.b_bf_nrm.p; s.bf_uv = (const float*)c.b_bf_uv.p; s.bf_idx = (const int32_t*)c.b_bf_idx.p;
  s.nodes = (const float*)c.b_nodes.p; s.tris = (const float*)c.b_tris.p;
  s.m_shade = (const float*)c.b_m_shade.p;
  if (!c.d_scene) HIP_TRY(hipMalloc(&c.d_scene, sizeof(DevScene)));
  HIP_TRY(hipMemcpy(c.d_scene, &s, sizeof(DevScene), hipMemcpyHostToDevice));
  return 0;
}

// What the trace kernels can address and walk (art_upload_scene, art_rebuild_device): nodes and triangles by 32-bit byte offsets (the
// 4-wide entry word keeps bit 31 for the leaf flag), quantised nodes for a 4-wide tree built on the GPU, at most kStackEntries on the stack.
int check_tree_limits(int width, int64_t n_nodes, int64_t n_tris, bool flat, bool gpu_built, bool have_qnodes, int stack) {
  const uint64_t off_limit = (width == 4) ? (1ull << 31) : (1ull << 32);
  if (flat && ((uint64_t)n_nodes * node_floats(width) * 4 >= (1ull << 32) || (uint64_t)n_tris * (width == 4 ? kQTriBytes : kTriBytes) >= off_limit))
    return fail("mesh too large: the trace kernel addresses nodes and triangles with 32-bit byte offsets (max ~33M triangles at width 4, ~89M at width 8)");
  if (width == 4 && n_nodes > 0 && gpu_built && !have_qnodes) return fail("internal: GPU build returned no quantised nodes");
  if (stack > kStackEntries) return fail("BVH traversal stack bound " + std::to_string(stack) + " exceeds " + std::to_string(kStackEntries));
  return 0;
}

void free_tree(GpuBvh& g) {
  for (void* p : {(void*)g.nodes, (void*)g.tris, g.qnodes}) if (p) (void)hipFree(p);
  g.nodes = nullptr; g.tris = nullptr; g.qnodes = nullptr;
}

void adopt_tree(Ctx& c, GpuBvh& g, int width) {
  c.b_nodes.release(); c.b_tris.release(); c.b_qnodes.release();
  c.b_qnodes.p = g.qnodes; c.b_qnodes.bytes = g.qnodes ? (size_t)g.n_nodes * kQNodeBytes : 0;
  c.b_nodes.p = g.nodes; c.b_nodes.bytes = (size_t)g.n_nodes * node_floats(width) * 4;
  c.b_tris.p = g.tris; c.b_tris.bytes = (size_t)g.n_tris * kTriFloats * 4;
  g.nodes = nullptr; g.qnodes = nullptr; g.tris = nullptr;                // (owned by the context now)
  c.bvh_stack_bound = std::max(8, g.max_stack);
  c.blocks_per_cu = 0;   // re-query occupancy
}

int pad_tri_records(DevBuf& dst, const float* tris, int n, hipStream_t s) {      // (the 4-wide kernel reads triangle records padded to 64 bytes)
  if (ensure(dst, (size_t)n * kQTriBytes)) return 1;
  launch_pad_tris(s, tris, (float*)dst.p, n);
  return hipGetLastError() == hipSuccess ? 0 : fail("padding the triangle records: kernel launch failed");
}

int upload_scene(const ArtSceneDesc* d) {
  if (!d) return fail("art_upload_scene: null scene");
  std::string err;
  HostScene hs;
  if (!flatten_scene(*d, g_devs[0].opt.bvh_params, hs, err)) return fail(err);      // validation + host BVH build: once, no GPU needed
  const std::vector<float> tri9 = std::move(hs.deferred_tri9);                    // option bvh_builder >= 1: every device builds its own tree
  hs.deferred_tri9.clear();
  Dev0Guard guard;
  reset_update_info();
  for (int k = 0; k < g_ndev; ++k) {                                              // scene + BVH replicated on every GPU
    if (use_dev(k)) return 1;
    Ctx& c = g_ctx;
    if (c.refit.ready || c.move.ready) HIP_TRY(hipStreamSynchronize(c.stream));  // (a refit or a move still in flight reads the plan)
    release_updates(c);
    c.opt.bvh_params = g_devs[0].opt.bvh_params;
    if (ensure_device()) return 1;
    int dev_stack = hs.bvh.max_stack;
    if (!tri9.empty()) {
      DevBuf t9;
      if (upload(t9, tri9)) return 1;
      GpuBvh g;
      const bool ok = build_bvh8_gpu((const float*)t9.p, (int)(tri9.size() / 9), c.opt.bvh_params, c.stream, g, err);
      t9.release();
      if (!ok) { free_tree(g); return fail("GPU BVH build: " + err); }
      adopt_tree(c, g, c.opt.bvh_params.width);
      dev_stack = g.max_stack;
      if (k == 0) {
        hs.bvh.width = c.opt.bvh_params.width;
        hs.bvh.n_nodes = g.n_nodes; hs.bvh.n_tris = g.n_tris; hs.bvh.max_stack = g.max_stack;
        hs.bvh_build_ms = g.build_ms; hs.gpu_built = true;
      }
      hs.hdr.n_nodes = g.n_nodes; hs.hdr.n_tris = g.n_tris;                       // node numbering may differ between devices (atomics), sizes do not
    }
    if (check_tree_limits(hs.hdr.node_width, hs.hdr.n_nodes, hs.hdr.n_tris, hs.hdr.n_inst == 0, hs.gpu_built, c.b_qnodes.p != nullptr, dev_stack)) return 1;
    if (upload_scene_arrays(hs)) return 1;
    c.b_qtris.release();
    // the 4-wide kernel's padded records: the flat tree's, or (instanced scene) the meshes' object-space records
    const bool inst = hs.hdr.n_inst > 0;
    const int nrec = inst ? (int)(hs.two.blas_tris.size() / kTriFloats) : (hs.hdr.node_width == 4 ? hs.hdr.n_tris : 0);
    if (nrec > 0) {
      if (pad_tri_records(c.b_qtris, (const float*)(inst ? c.b_blas_tris.p : c.b_tris.p), nrec, c.stream)) return 1;
      HIP_TRY(hipStreamSynchronize(c.stream));
    }
    c.bvh_stack_bound = std::max(8, dev_stack);
    c.blocks_per_cu = 0;   // re-query occupancy
    c.scene_ready = true;
    c.trial.reset();     // a new scene: the shade stage measures its items-per-thread choice again
  }
  g_devs[0].host_scene = std::move(hs);
  return 0;
}

// ------------------------------------------------------------------------------------------------
int build_shard() {
  Ctx& c = g_ctx;
  const std::vector<uint32_t> pm = build_pixmap(c.width, c.height, c.rank, c.nranks, c.tile);
  c.npix_local = (int)pm.size();
  // Stream-ordered through a pinned copy, and b_pixmap only ever grows: art_resize and art_set_shard return without waiting for the
  // stream.  (Freeing and allocating b_pixmap on every call, as upload() does, made both wait until EVERY stream of the device was idle
  // -- hipFree does -- so a caller's work queued on the stream held the host up: tests/test_gpu_bound_accum.py, the stream test.)
  // The list is read by the passes that follow on the same stream; a pass before it has been waited for by its own call.
  if (pm.empty()) return 0;
  const size_t bytes = pm.size() * sizeof(uint32_t);
  if (c.pixmap_copied) HIP_TRY(hipEventSynchronize(c.pixmap_copied));      // (the pinned copy's previous upload: it is about to be overwritten)
  else HIP_TRY(hipEventCreateWithFlags(&c.pixmap_copied, hipEventDisableTiming));
  if (c.pixmap_host_bytes < bytes) {
    if (c.pixmap_host) { (void)hipHostFree(c.pixmap_host); c.pixmap_host = nullptr; c.pixmap_host_bytes = 0; }
    HIP_TRY(hipHostMalloc((void**)&c.pixmap_host, bytes, hipHostMallocDefault));
    c.pixmap_host_bytes = bytes;
  }
  if (ensure(c.b_pixmap, bytes)) return 1;
  std::memcpy(c.pixmap_host, pm.data(), bytes);
  HIP_TRY(hipMemcpyAsync(c.b_pixmap.p, c.pixmap_host, bytes, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipEventRecord(c.pixmap_copied, c.stream));
  return 0;
}

static int resize_one(int w, int h) {
  Ctx& c = g_ctx;
  if (ensure_device()) return 1;
  if (!c.pass_clock.empty()) HIP_TRY(hipStreamSynchronize(c.stream));      // (host callbacks of earlier passes still write into their cells)
  c.width = w; c.height = h;
  const size_t n = (size_t)w * h;
  if (ensure(c.b_accum, n * 12) || ensure(c.b_screen, n * 4)) return 1;
  float* acc = c.ext_accum ? c.ext_accum : (float*)c.b_accum.p;
  HIP_TRY(hipMemsetAsync(acc, 0, n * 12, c.stream));
  if (c.ext_moments) HIP_TRY(hipMemsetAsync(c.ext_moments, 0, n * 8, c.stream));
  c.spp = 0;
  c.stats = ArtStats();
  c.stage = ArtStageStats();
  c.trial.reset();                                       // (the batch size follows the frame: measure again)
  c.lost_reported = 0;                                   // (the device counters are zeroed below)
  if (c.d_items) HIP_TRY(hipMemsetAsync(c.d_items, 0, 32 * sizeof(unsigned long long), c.stream));
  c.camera_traced = 0;
  HIP_TRY(hipMemsetAsync(c.d_counters, 0, kCounters * sizeof(unsigned long long), c.stream));
  return build_shard();
}
int resize(int w, int h) {
  if (w <= 0 || h <= 0 || (int64_t)w * h > (1ll << 30)) return fail("art_resize: bad size");
  if (each_device(/*stop_at_failure=*/true, [&](int) { return resize_one(w, h); })) return 1;
  for (int k = 0; k < g_ndev; ++k) { Ctx& c = g_devs[k]; c.busy_ms = c.idle_ms = c.start_skew_ms = 0.0; for (Ctx::PassClock* pc : c.pass_clock) delete pc; c.pass_clock.clear(); }
  if (g_devs[0].device_ready && !use_dev(0)) reset_reduce_info();
  return 0;
}

// drain event pairs into stats (requires the stream to be idle)
static int collect_timing() {
  Ctx& c = g_ctx;
  HIP_TRY(c.stage_pairs.fold(/*wait=*/true, [&c](float ms, uint8_t tagged) {
    const ShadeTrial::Tag tag = ShadeTrial::decode(tagged);
    if (tag.kind == 0) { c.stats.trace_ms += ms; c.stats.trace_launches += 1; }
    else if (tag.kind == 1) { c.stage.shade_ms += ms; c.stage.shade_launches += 1; c.trial.add(tag.trial, tag.gen, ms); }
    else if (tag.kind == 2) c.stage.raygen_ms += ms;
    else c.stage.fold_ms += ms;
  }));
  // both trial batches are done (the stream is idle): the faster setting is kept from here on
  if (c.trial.decide() && g_debug_addr) std::fprintf(stderr, "ART_DEBUG_ADDR shade_per trial: 4 items per thread %.3f ms, 2 items per thread %.3f ms per batch of %lld paths -> %d\n", c.trial.ms[0], c.trial.ms[1], (long long)c.trial.P[0], c.trial.per);
  if (c.d_items) {
    unsigned long long it[32];
    HIP_TRY(hipMemcpy(it, c.d_items, sizeof it, hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) { c.stage.items_in[k] = it[k]; c.stage.items_out[k] = it[16 + k]; }
  }
  unsigned long long cnt[kCounters];
  HIP_TRY(hipMemcpy(cnt, c.d_counters, sizeof cnt, hipMemcpyDeviceToHost));
  c.stats.node_phase_iters = cnt[CNT_NODE_ITERS]; c.stats.leaf_phase_iters = cnt[CNT_LEAF_ITERS]; c.stats.wave_iters = cnt[CNT_WAVE_ITERS];
  c.stats.rays = cnt[CNT_RAYS];
  c.stats.lost_paths = cnt[CNT_LOST];
  c.stats.box_tests = cnt[CNT_STATS]; c.stats.tri_tests = cnt[CNT_STATS + 1]; c.stats.node_visits = cnt[CNT_STATS + 2]; c.stats.leaf_visits = cnt[CNT_STATS + 3]; c.stats.traced_rays = cnt[CNT_TRACED];
  return 0;
}

int synchronize_one() {
  Ctx& c = g_ctx;
  if (!c.device_ready) return 0;
  HIP_TRY(hipStreamSynchronize(c.stream));
  HIP_TRY(c.pass_pairs.fold(/*wait=*/true, [&c](float ms, uint8_t) { c.stats.pass_ms += ms; }));
  if (collect_timing()) return 1;
  if (sync_updates()) return 1;
  // a lost path is a wrong picture, not a statistic -- a stage that found a path without an output item, a ray its bank has no
  // record for, a material its instantiation was not compiled for, or a staged trace record that did not name the hit slot its position
  // implies (art_shade.h emit_ray) fails the call that waits for the render
  // (the baseline is lost_reported, which only this function advances -- collect_timing may run any number of times between
  // two synchronises without absorbing a loss)
  if (c.stats.lost_paths != c.lost_reported) {
    const uint64_t n = c.stats.lost_paths - c.lost_reported;
    c.lost_reported = c.stats.lost_paths;
    return fail("render self-check: " + std::to_string(n) + " path(s) lost by the wavefront stages (ArtStats::lost_paths); the image is not valid");
  }
  return 0;
}
int synchronize() {
  const int rc = each_device(/*stop_at_failure=*/false, [](int) { return synchronize_one(); });      // (every device is waited for and checked, also after a failure on one)
  if (g_devs[0].device_ready && !use_dev(0)) fold_reduce_events();
  return rc;
}

// every pixel has one owner, so the other devices hold exact zeros there and the sum over devices is exact: ONE
// ncclReduce(sum, float32, W*H*3, root = device 0) over xGMI, grouped over the process' communicators, each on its device's stream
// (ordered after that device's render kernels).  The per-device buffers stay as they are (they keep accumulating over passes); the
// sum lands in device 0's b_reduced.  Several contexts on ONE physical GPU (rehearsal on a 1-GPU box) cannot form a communicator:
// there the sum is a chain of local adds in device order, which is the same exact sum.
static int reduce_accum(const float** out) {
  Ctx& c0 = g_devs[0];
  if (g_ndev == 1 && !g_comms_ready) { *out = c0.ext_accum ? c0.ext_accum : (const float*)c0.b_accum.p; return 0; }
  const size_t count = (size_t)c0.width * c0.height * 3;
  Dev0Guard guard;
  if (use_dev(0) || ensure(c0.b_reduced, count * 4)) return 1;
  EventPairs::Timer timer;                   // around the reduce, ended on every way out (synchronize() folds the pairs)
  HIP_TRY(g_reduce_pairs.begin(timer, c0.stream));
  g_reduces += 1; g_reduce_path = g_comms_ready ? 1 : 2;
  if (g_comms_ready) {
    if (ncclGroupStart() != ncclSuccess) return fail("ncclGroupStart failed");
    for (int k = 0; k < g_ndev; ++k) {
      const ncclResult_t r = ncclReduce(g_devs[k].b_accum.p, k == 0 ? c0.b_reduced.p : nullptr, count, ncclFloat32, ncclSum, 0, g_comms[k], g_devs[k].stream);
      if (r != ncclSuccess) { (void)ncclGroupEnd(); return fail(std::string("ncclReduce: ") + ncclGetErrorString(r)); }
    }
    const ncclResult_t r = ncclGroupEnd();
    if (r != ncclSuccess) return fail(std::string("ncclGroupEnd: ") + ncclGetErrorString(r));
  } else if (g_same_gpu) {
    HIP_TRY(hipMemcpyAsync(c0.b_reduced.p, c0.b_accum.p, count * 4, hipMemcpyDeviceToDevice, c0.stream));
    for (int k = 1; k < g_ndev; ++k) {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(e, g_devs[k].stream));
      HIP_TRY(hipStreamWaitEvent(c0.stream, e, 0));
      (void)hipEventDestroy(e);
      launch_add_f32(c0.stream, (const float*)g_devs[k].b_accum.p, (float*)c0.b_reduced.p, count);
    }
    // the adds read every context's accum on c0.stream: a later render pass on stream k must not overwrite it before they are done
    hipEvent_t done;
    HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(done, c0.stream));
    for (int k = 1; k < g_ndev; ++k) HIP_TRY(hipStreamWaitEvent(g_devs[k].stream, done, 0));
    (void)hipEventDestroy(done);
  } else return fail("internal: multi-device mode without a reduce path");
  *out = (const float*)c0.b_reduced.p;
  return 0;
}

int download(float* accum_host, uint32_t* screen_host, int layout, int spp) {
  Ctx& c = g_ctx;
  if (c.width <= 0) return fail("no viewport");
  const float* acc = nullptr;
  if (reduce_accum(&acc)) return 1;
  return download_from(acc, accum_host, screen_host, layout, spp);
}

int download_from(const float* acc_dev, float* accum_host, uint32_t* screen_host, int layout, int spp) {
  Ctx& c = g_ctx;
  const int W = c.width, H = c.height; const size_t n = (size_t)W * H;
  if (screen_host) launch_resolve(c.stream, acc_dev, (int)n, 1.0f / (float)spp, (uint32_t*)c.b_screen.p);
  if (layout == ART_LAYOUT_ADA_XY) {
    if (ensure(c.b_stage, n * 12)) return 1;
    if (accum_host) {
      launch_to_xmajor_f3(c.stream, acc_dev, (float*)c.b_stage.p, W, H);
      HIP_TRY(hipMemcpyAsync(accum_host, c.b_stage.p, n * 12, hipMemcpyDeviceToHost, c.stream));
      HIP_TRY(hipStreamSynchronize(c.stream));
    }
    if (screen_host) {
      launch_to_xmajor_u32(c.stream, (const uint32_t*)c.b_screen.p, (uint32_t*)c.b_stage.p, W, H);
      HIP_TRY(hipMemcpyAsync(screen_host, c.b_stage.p, n * 4, hipMemcpyDeviceToHost, c.stream));
    }
  } else {
    if (accum_host) HIP_TRY(hipMemcpyAsync(accum_host, acc_dev, n * 12, hipMemcpyDeviceToHost, c.stream));
    if (screen_host) HIP_TRY(hipMemcpyAsync(screen_host, c.b_screen.p, n * 4, hipMemcpyDeviceToHost, c.stream));
  }
  HIP_TRY(hipStreamSynchronize(c.stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

// c's tree as it lies in HBM (c's GPU is current), after its stream has drained: a refit on another stream is ordered before that
static int fetch_tree(Ctx& c, std::vector<float>& nodes, std::vector<float>& tris) {
  const Bvh8& b = c.host_scene.bvh;
  HIP_TRY(hipStreamSynchronize(c.stream));
  nodes.resize((size_t)b.n_nodes * node_floats(b.width)); tris.resize((size_t)b.n_tris * kTriFloats);
  HIP_TRY(hipMemcpy(nodes.data(), c.b_nodes.p, nodes.size() * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tris.data(), c.b_tris.p, tris.size() * 4, hipMemcpyDeviceToHost));
  return 0;
}

// the uploaded tree of device 0 as host arrays (the packets art_export_bvh returns; that call keeps what it fetches, this one does not); the caller holds g_mu
int fetch_host_bvh(std::vector<float>& nodes, std::vector<float>& tris, int& width, int& n_tris) {
  Ctx& c = g_devs[0];
  if (!c.scene_ready) return fail("no scene uploaded");
  const Bvh8& b = c.host_scene.bvh;
  width = b.width; n_tris = b.n_tris;
  if (c.host_scene.tree_in_hbm_only() && b.nodes.empty()) return use_dev(0) || fetch_tree(c, nodes, tris);
  nodes = b.nodes; tris = b.tris;
  return 0;
}

void shutdown() {
  if (g_devs[0].device_ready && !use_dev(0)) { reset_reduce_info(); g_reduce_pairs.destroy(); }
  if (g_comms_ready) { for (int k = 0; k < g_ndev; ++k) (void)ncclCommDestroy(g_comms[k]); g_comms_ready = false; }
  g_same_gpu = false; g_multi_api = false;
  for (int k = g_ndev - 1; k >= 0; --k) {
    g_cur = &g_devs[k];
    Ctx& c = g_ctx;
    if (c.device_ready) {
      if (c.device >= 0) (void)hipSetDevice(c.device);
      (void)hipDeviceSynchronize();
      DevBuf* bufs[] = {&c.b_spheres, &c.b_sphere_mat, &c.b_lights, &c.b_materials, &c.b_bf_pos, &c.b_bf_nrm, &c.b_bf_uv, &c.b_bf_idx,
                        &c.b_nodes, &c.b_qnodes, &c.b_tris, &c.b_qtris, &c.b_m_shade, &c.b_accum, &c.b_screen, &c.b_stage,
                        &c.b_pixmap, &c.b_paths, &c.b_rays, &c.b_ids, &c.b_queue, &c.b_ovf,
                        &c.b_inst, &c.b_tlas_nodes, &c.b_tlas_tris, &c.b_blas_nodes, &c.b_blas_tris, &c.b_query, &c.b_denoise, &c.b_select, &c.b_masklist};
      for (DevBuf* b : bufs) b->release();
      for (void* p : {(void*)c.d_cursor, (void*)c.d_scene, (void*)c.d_counters, (void*)c.d_live, (void*)c.d_items}) if (p) (void)hipFree(p);
      c.stage_pairs.destroy(); c.pass_pairs.destroy(); c.rebuild_pairs.destroy();
      for (hipEvent_t e : c.q_ev) if (e) (void)hipEventDestroy(e);
      if (c.pixmap_copied) (void)hipEventDestroy(c.pixmap_copied);
      if (c.pixmap_host) (void)hipHostFree(c.pixmap_host);
      destroy_updates(c);
      for (Ctx::PassClock* pc : c.pass_clock) delete pc;      // (after hipDeviceSynchronize: no callback is pending)
      c.b_reduced.release();
      if (c.own_stream) (void)hipStreamDestroy(c.own_stream);
    }
    c = Ctx();
  }
  g_ndev = 1; g_cur = &g_devs[0];
}

}  // namespace art

// ================================================================================================
using namespace art;

extern "C" {

int art_init(int device_ordinal) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_ctx.device_ready && device_ordinal >= 0 && device_ordinal != g_ctx.device) return fail("art_init: already bound to another device; call art_shutdown first");
  g_ctx.device = device_ordinal;
  if (const char* e = getenv("ART_TRACE_KERNEL")) g_ctx.opt.trace_kernel = (std::strcmp(e, "simple") == 0) ? TRACE_SIMPLE : TRACE_COOP;
  if (const char* e = getenv("ART_BATCH_PATHS")) g_ctx.opt.batch_paths = std::min<int64_t>(1ll << 27, std::max<int64_t>(1024, atoll(e)));
  return ensure_device();
}

// One process, n GPUs (SURVEY 8e / 8b "Threading": the Ada host calls Render_Pass from its environment task, test.adb:50, so the
// fan-out over the node's GPUs has to happen below the C ABI).  ordinals == NULL: devices 0..n-1.  Every device gets its own
// context, stream, replicated scene and path buffers; device k owns the 32x32 pixel tiles (bx, by) with (bx + 3 by) mod n == k (diagonals: build_pixmap); art_render_pass /
// art_download add the float3 framebuffers into device 0 with ONE RCCL reduce over xGMI.  Listing the same ordinal several times puts
// several contexts on one GPU (a rehearsal of the whole path on a 1-GPU box; the reduce is then a local sum).
int art_init_devices(int32_t n, const int32_t* ordinals) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (n < 1 || n > kMaxDevices) return fail("art_init_devices: 1.." + std::to_string(kMaxDevices) + " devices");
  for (int k = 0; k < kMaxDevices; ++k) if (g_devs[k].device_ready) return fail("art_init_devices: already initialised; call art_shutdown first");
  int avail = 0;
  hipError_t e = hipGetDeviceCount(&avail);
  if (e != hipSuccess || avail <= 0) return fail("no HIP device available (this library has no CPU path): " + std::string(hipGetErrorString(e)));
  int ord[kMaxDevices]; bool distinct = true, same = true;
  for (int k = 0; k < n; ++k) {
    ord[k] = ordinals ? ordinals[k] : k;
    if (ord[k] < 0 || ord[k] >= avail) return fail("art_init_devices: device " + std::to_string(ord[k]) + " does not exist (" + std::to_string(avail) + " visible)");
    for (int i = 0; i < k; ++i) { if (ord[i] == ord[k]) distinct = false; else same = false; }
  }
  if (n > 1 && !distinct && !same) return fail("art_init_devices: the ordinals must be all different (one context per GPU) or all equal (rehearsal on one GPU)");
  const Options opts = g_devs[0].opt;               // options set before initialisation apply to every device
  Dev0Guard guard;
  g_ndev = n;
  for (int k = 0; k < n; ++k) {
    Ctx& c = g_devs[k];
    c = Ctx();
    c.opt = opts;
    c.device = ord[k]; c.rank = k; c.nranks = n; c.tile = 32;
    if (use_dev(k) || ensure_device()) { shutdown(); return 1; }
    if (n > 1) {
      if (hipStreamCreateWithFlags(&c.own_stream, hipStreamNonBlocking) != hipSuccess) { shutdown(); return fail("hipStreamCreate failed"); }
      c.stream = c.own_stream;
    }
  }
  // ART_FORCE_RCCL=1: build the communicator for a single device too, so that a 1-GPU box exercises the very RCCL calls of the n-GPU path
  const bool force_rccl = (n == 1) && getenv("ART_FORCE_RCCL") && std::atoi(getenv("ART_FORCE_RCCL")) != 0;
  if ((n > 1 && distinct) || force_rccl) {
    const ncclResult_t r = ncclCommInitAll(g_comms, n, ord);
    if (r != ncclSuccess) { shutdown(); return fail(std::string("ncclCommInitAll: ") + ncclGetErrorString(r)); }
    g_comms_ready = true;
  }
  g_same_gpu = (n > 1 && !distinct);
  g_multi_api = true;
  return 0;
}

int32_t art_device_count(void) { std::lock_guard<std::mutex> lk(g_mu); return g_ndev; }

#define SINGLE_DEVICE_ONLY(name) if (g_ndev > 1) return fail(name ": not available after art_init_devices(n > 1); the library shards and reduces by itself")

int art_set_stream(void* hip_stream) { std::lock_guard<std::mutex> lk(g_mu); SINGLE_DEVICE_ONLY("art_set_stream"); g_ctx.stream = (hipStream_t)hip_stream; return 0; }

int art_upload_scene(const ArtSceneDesc* scene) { std::lock_guard<std::mutex> lk(g_mu); return upload_scene(scene); }

int art_resize(int32_t w, int32_t h) { std::lock_guard<std::mutex> lk(g_mu); return resize(w, h); }

int art_set_shard(int32_t rank, int32_t nranks, int32_t tile) {
  std::lock_guard<std::mutex> lk(g_mu);
  SINGLE_DEVICE_ONLY("art_set_shard");
  if (nranks < 1 || rank < 0 || rank >= nranks || tile < 1) return fail("art_set_shard: bad arguments");
  g_ctx.rank = rank; g_ctx.nranks = nranks; g_ctx.tile = tile;
  if (g_ctx.width > 0) return build_shard();
  return 0;
}

int art_render_pass(const ArtPassParams* p, float* accum_host, uint32_t* screen_host, int32_t* spp_inout) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (render_pass_device(p, spp_inout)) return 1;
  if (accum_host || screen_host) { if (download(accum_host, screen_host, p->layout, g_ctx.spp)) return 1; }
  return synchronize();
}

int art_debug_hit_pass(const ArtPassParams* p, float* accum_host, uint32_t* screen_host, int32_t* prim_index, int32_t* mat_id, int32_t* prim_type) {
  std::lock_guard<std::mutex> lk(g_mu);
  return debug_pass(p, accum_host, screen_host, prim_index, mat_id, prim_type);
}

int art_bind_accum(void* device_accum_rowmajor) {
  std::lock_guard<std::mutex> lk(g_mu);
  SINGLE_DEVICE_ONLY("art_bind_accum");
  // (the frame may not be known yet, so only the kind of memory and its device are checked: a refused pointer leaves the binding as it was)
  if (device_accum_rowmajor && (ensure_device() || check_planes({{device_accum_rowmajor, 0, "art_bind_accum: device_accum_rowmajor"}}))) return 1;
  g_ctx.ext_accum = (float*)device_accum_rowmajor;
  return 0;
}
int art_bind_moments(void* device_moments_rowmajor) {
  std::lock_guard<std::mutex> lk(g_mu);
  SINGLE_DEVICE_ONLY("art_bind_moments");
  // (as art_bind_accum: only the kind of memory and its device can be checked here; a refused pointer leaves the binding as it was)
  if (device_moments_rowmajor && (ensure_device() || check_planes({{device_moments_rowmajor, 0, "art_bind_moments: device_moments_rowmajor"}}))) return 1;
  g_ctx.ext_moments = (float*)device_moments_rowmajor;
  return 0;
}
void* art_accum_device(void) {          // device 0; in multi-device mode the reduced framebuffer (valid after a reduce: art_reduce / art_download)
  std::lock_guard<std::mutex> lk(g_mu);
  return (g_ndev > 1) ? g_devs[0].b_reduced.p : (void*)accum_ptr();
}

// multi-device: enqueue the framebuffer reduce to device 0 (bench.py times it inside its step loop); no-op with one device
int art_reduce(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  const float* acc = nullptr;
  return reduce_accum(&acc);
}

int art_download(float* accum_host, uint32_t* screen_host, int32_t layout, int32_t spp) {
  std::lock_guard<std::mutex> lk(g_mu);
  // 1 / spp scales the resolve only: without a screen spp is not read; with one, spp <= 0 would divide by zero or negate the picture
  if (screen_host && spp <= 0) return fail("art_download: spp must be positive to resolve a screen, got " + std::to_string(spp));
  return download(accum_host, screen_host, layout, spp);
}

int art_synchronize(void) { std::lock_guard<std::mutex> lk(g_mu); return synchronize(); }

int art_trace_rays(const float* origins, const float* dirs, const float* tfar, int64_t n, ArtHit* out, int32_t kernel, ArtStats* stats) {
  std::lock_guard<std::mutex> lk(g_mu);          // ray queries run on device 0
  return trace_rays(origins, dirs, tfar, n, out, kernel, stats);
}

int art_trace_rays_device(const float* origins3f, const float* dirs3f, const float* tnear, const float* tfar, int64_t n, ArtHit* hits_out, int32_t kernel, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // ray queries run on device 0
  if (!hits_out && n > 0) return fail("art_trace_rays_device: null hits_out");
  return query_rays(origins3f, dirs3f, tnear, tfar, n, hits_out, nullptr, kernel, (hipStream_t)hip_stream);
}

int art_occluded_rays_device(const float* origins3f, const float* dirs3f, const float* tnear, const float* tfar, int64_t n, uint8_t* occluded_out, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!occluded_out && n > 0) return fail("art_occluded_rays_device: null occluded_out");
  return query_rays(origins3f, dirs3f, tnear, tfar, n, nullptr, occluded_out, TRACE_COOP, (hipStream_t)hip_stream);
}

int art_render_aovs_device(const ArtPassParams* p, const ArtAovBuffers* out, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return render_aovs(p, out, (hipStream_t)hip_stream);
}

int art_render_aovs_motion_device(const ArtPassParams* p, const ArtAovBuffers* out, const ArtMotionSource* src, float* motion3f, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return render_aovs(p, out, (hipStream_t)hip_stream, motion3f ? src : nullptr, motion3f);
}

int art_aovs_rays_device(const ArtAovRaysParams* p, const float* origins3f, const float* dirs3f, const float* tnear, const float* tfar, int64_t n_rays,
                         const ArtAovRayBuffers* out, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  SINGLE_DEVICE_ONLY("art_aovs_rays_device");
  return aovs_rays(p, origins3f, dirs3f, tnear, tfar, n_rays, out, (hipStream_t)hip_stream);
}

int art_camera_rays_device(const ArtPassParams* p, float* origins3f, float* dirs3f, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like art_render_aovs_device, on device 0
  return camera_rays(p, origins3f, dirs3f, (hipStream_t)hip_stream);
}

int art_denoise_device(const ArtDenoiseParams* p, const float* color3f, const float* albedo3f, const float* normal3f, const float* depth, float* out3f, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return denoise_device(p, color3f, albedo3f, normal3f, depth, out3f, (hipStream_t)hip_stream);
}

int art_denoise_svgf_device(const ArtSvgfParams* p, const float* color3f, const float* moments2f, const float* albedo3f, const float* normal3f, const float* depth,
                            float* out3f, float* variance_out, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return denoise_svgf_device(p, color3f, moments2f, albedo3f, normal3f, depth, out3f, variance_out, (hipStream_t)hip_stream);
}

int art_denoise_svgf_var_device(const ArtSvgfParams* p, const float* color3f, const float* variance1f, const float* albedo3f, const float* normal3f, const float* depth,
                                float* out3f, float* variance_out, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return denoise_svgf_device(p, color3f, variance1f, albedo3f, normal3f, depth, out3f, variance_out, (hipStream_t)hip_stream, true);
}

int art_temporal_device(const ArtTemporalParams* p, const float* color3f, const float* moments2f, const float* normal3f, const float* depth, const int32_t* id,
                        const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return temporal_device(p, color3f, moments2f, normal3f, depth, id, hist_in, hist_out, out3f, variance_out, length_out, (hipStream_t)hip_stream);
}

int art_temporal_motion_device(const ArtTemporalParams* p, const float* color3f, const float* moments2f, const float* normal3f, const float* depth, const int32_t* id,
                               const float* motion3f, const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return temporal_device(p, color3f, moments2f, normal3f, depth, id, hist_in, hist_out, out3f, variance_out, length_out, (hipStream_t)hip_stream, motion3f,
                         motion3f ? "art_temporal_motion_device" : "art_temporal_device");
}

int art_compact_mask_device(const uint8_t* mask1b, uint32_t* pixels_out, int64_t cap, uint32_t* count_out, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return compact_mask_device(mask1b, pixels_out, cap, count_out, (hipStream_t)hip_stream);
}

int art_render_pass_masked(const ArtPassParams* p, const uint8_t* mask1b, uint32_t* counts1u, int32_t* spp_inout, int64_t* pixels_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  SINGLE_DEVICE_ONLY("art_render_pass_masked");
  if (render_pass_masked(p, mask1b, counts1u, spp_inout, pixels_out)) return 1;
  return synchronize();
}

int art_radiance_rays_device(const ArtRadianceParams* p, const float* origins3f, const float* dirs3f, const uint32_t* keys1u, int64_t n,
                             float* radiance3f, float* moments2f) {
  std::lock_guard<std::mutex> lk(g_mu);
  SINGLE_DEVICE_ONLY("art_radiance_rays_device");
  if (radiance_rays(p, origins3f, dirs3f, keys1u, n, radiance3f, moments2f)) return 1;
  return synchronize();
}

int art_adaptive_estimate_device(const ArtAdaptiveParams* p, const float* accum3f, const float* moments2f, const uint32_t* counts1u,
                                 float* mean3f, float* variance1f, float* error1f, uint8_t* mask1b, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return adaptive_estimate_device(p, accum3f, moments2f, counts1u, mean3f, variance1f, error1f, mask1b, (hipStream_t)hip_stream);
}

int art_svgf_spatial_variance_device(const ArtSvgfSpatialParams* p, const void* hist, const float* variance_in1f, float* variance_out1f, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return svgf_spatial_variance_device(p, hist, variance_in1f, variance_out1f, (hipStream_t)hip_stream);
}

int64_t art_exposure_state_bytes(void) { return 4 * (4 + 256); }      // (the header's layout: four words and the 256 bins)

int art_auto_exposure_device(const ArtExposureParams* p, const float* color3f, void* state, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return auto_exposure_device(p, color3f, state, (hipStream_t)hip_stream);
}

int art_display_device(const ArtDisplayParams* p, const float* color3f, const void* exposure_state, uint32_t* screen1u, float* ldr3f, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return display_device(p, color3f, exposure_state, screen1u, ldr3f, (hipStream_t)hip_stream);
}

int art_upsample_device(const ArtUpsampleParams* p, const float* lo_color3f, const ArtUpsampleGuides* lo, const ArtUpsampleGuides* hi, float* out3f, uint8_t* fallback1b,
                        void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return upsample_device(p, lo_color3f, lo, hi, out3f, fallback1b, (hipStream_t)hip_stream);
}

int art_temporal_upsample_device(const ArtTemporalUpsampleParams* p, const float* lo_color3f, const float* lo_moments2f, const ArtTemporalUpsampleGuides* lo,
                                 const ArtTemporalUpsampleGuides* hi, const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out,
                                 uint8_t* fallback1b, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return temporal_upsample_device(p, lo_color3f, lo_moments2f, lo, hi, hist_in, hist_out, out3f, variance_out, length_out, fallback1b, (hipStream_t)hip_stream);
}

int art_firefly_device(const ArtFireflyParams* p, const float* color3f, const float* moments2f, const int32_t* id, float* out3f, float* moments_out2f, uint8_t* clamped1b,
                       void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return firefly_device(p, color3f, moments2f, id, out3f, moments_out2f, clamped1b, (hipStream_t)hip_stream);
}

int art_bloom_device(const ArtBloomParams* p, const float* color3f, const void* exposure_state, float* out3f, float* bloom3f, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);          // like the ray queries, on device 0
  return bloom_device(p, color3f, exposure_state, out3f, bloom3f, (hipStream_t)hip_stream);
}

int64_t art_temporal_history_bytes(int32_t width, int32_t height) {
  if (width < 1 || height < 1 || (int64_t)width * height > (1ll << 28)) return 0;
  return 48 * (int64_t)width * height;
}

int art_set_camera(const float cam_pos[3], const float cam_matrix[16]) { std::lock_guard<std::mutex> lk(g_mu); return set_camera(cam_pos, cam_matrix); }

int art_refit_device(const float* pos3f, const float* nrm3f, int64_t nverts, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return refit_device(pos3f, nrm3f, nverts, (hipStream_t)hip_stream);
}

int art_get_refit_info(ArtRefitInfo* out) { std::lock_guard<std::mutex> lk(g_mu); return get_refit_info(out); }

int art_rebuild_device(const float* pos3f, const float* nrm3f, int64_t nverts, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return rebuild_device(pos3f, nrm3f, nverts, (hipStream_t)hip_stream);
}

int art_get_rebuild_info(ArtRebuildInfo* out) { std::lock_guard<std::mutex> lk(g_mu); return get_rebuild_info(out); }

int art_get_tree_cost(ArtTreeCost* out) { std::lock_guard<std::mutex> lk(g_mu); return get_tree_cost(out); }

int art_move_instances_device(const float* m12f, int64_t n_instances, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return move_instances_device(m12f, n_instances, (hipStream_t)hip_stream);
}

int art_get_move_info(ArtMoveInfo* out) { std::lock_guard<std::mutex> lk(g_mu); return get_move_info(out); }

int art_refit_mesh_device(int32_t mesh, const float* pos3f, const float* nrm3f, int64_t nverts, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return refit_mesh_device(mesh, pos3f, nrm3f, nverts, (hipStream_t)hip_stream);
}

int art_get_mesh_refit_info(ArtMeshRefitInfo* out) { std::lock_guard<std::mutex> lk(g_mu); return get_mesh_refit_info(out); }

int art_rebuild_instance_tree_device(void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return rebuild_instance_tree_device((hipStream_t)hip_stream);
}

int art_get_instance_rebuild_info(ArtInstanceRebuildInfo* out) { std::lock_guard<std::mutex> lk(g_mu); return get_instance_rebuild_info(out); }

int art_get_instance_tree_cost(ArtTreeCost* out) { std::lock_guard<std::mutex> lk(g_mu); return get_instance_tree_cost(out); }

int art_rebuild_mesh_tree_device(int32_t mesh, void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return rebuild_mesh_tree_device(mesh, (hipStream_t)hip_stream);
}

int art_get_mesh_rebuild_info(ArtMeshRebuildInfo* out) { std::lock_guard<std::mutex> lk(g_mu); return get_mesh_rebuild_info(out); }

int art_get_mesh_tree_cost(int32_t mesh, ArtTreeCost* out) { std::lock_guard<std::mutex> lk(g_mu); return get_mesh_tree_cost(mesh, out); }

int art_export_two_level(ArtTwoLevelInfo* info, const ArtTwoLevelBuffers* buf) { std::lock_guard<std::mutex> lk(g_mu); return export_two_level(info, buf); }

int art_export_bvh(float* nodes, int64_t node_cap, float* tris, int64_t tri_cap, ArtBvhInfo* info) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_ctx.scene_ready) return fail("no scene uploaded");
  Bvh8& b = g_ctx.host_scene.bvh;
  if (g_ctx.scene.n_inst > 0 && (nodes || tris)) return fail("art_export_bvh: an instanced scene has a two-level tree; only its sizes are reported here (ArtBvhInfo); art_export_two_level exports its arrays");
  if (g_ctx.host_scene.tree_in_hbm_only() && b.nodes.empty() && (nodes || tris) && fetch_tree(g_ctx, b.nodes, b.tris)) return 1;     // a GPU-built or refitted tree is fetched on first request, and kept
  if (info) { info->n_nodes = b.n_nodes; info->n_tris = b.n_tris; info->max_stack = b.max_stack; info->node_width = b.width; info->build_ms = g_ctx.host_scene.bvh_build_ms; }
  if (nodes) { if (node_cap < (int64_t)b.nodes.size()) return fail("art_export_bvh: node buffer too small"); std::memcpy(nodes, b.nodes.data(), b.nodes.size() * 4); }
  if (tris) { if (tri_cap < (int64_t)b.tris.size()) return fail("art_export_bvh: triangle buffer too small"); std::memcpy(tris, b.tris.data(), b.tris.size() * 4); }
  return 0;
}

int art_get_reduce_info(ArtReduceInfo* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!out) return fail("null ArtReduceInfo");
  if (synchronize()) return 1;
  std::memset(out, 0, sizeof *out);
  out->devices = g_ndev;
  if (g_comms_ready) { int n = 0; if (ncclCommCount(g_comms[0], &n) != ncclSuccess) return fail("ncclCommCount failed"); out->rccl_ranks = n; }
  fold_pass_clocks();                      // (synchronize() above folded the reduces' event pairs and left every stream idle)
  out->path = g_reduce_path; out->reduces = g_reduces; out->reduce_ms = g_reduce_ms;
  for (int k = 0; k < g_ndev && k < 8; ++k) {
    const Ctx& c = g_devs[k];
    out->device_pass_ms[k] = c.stats.pass_ms; out->device_busy_ms[k] = c.busy_ms; out->device_idle_ms[k] = c.idle_ms; out->device_start_skew_ms[k] = c.start_skew_ms;
  }
  out->passes = g_passes; out->passes_overlapped = g_passes_overlapped;
  return 0;
}

int art_get_stage_stats(ArtStageStats* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!out) return fail("null ArtStageStats");
  if (synchronize()) return 1;
  *out = g_devs[0].stage;
  return 0;
}

int art_get_stats(ArtStats* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!out) return fail("null stats");
  if (synchronize()) return 1;
  *out = g_devs[0].stats;                 // trace_ms / trace_launches / wave counters: device 0's (per-device quantities)
  for (int k = 1; k < g_ndev; ++k) {      // work counters: the whole job
    const ArtStats& t = g_devs[k].stats;
    out->rays += t.rays; out->samples += t.samples; out->box_tests += t.box_tests; out->tri_tests += t.tri_tests;
    out->node_visits += t.node_visits; out->leaf_visits += t.leaf_visits; out->traced_rays += t.traced_rays;
    out->lost_paths += t.lost_paths;      // the compacted work set's self-check ("must stay 0") covers every device
    out->pass_ms = std::max(out->pass_ms, t.pass_ms);
  }
  return 0;
}

int art_get_camera_rays_traced(uint64_t* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!out) return fail("null camera ray count");
  *out = 0;
  for (int k = 0; k < g_ndev; ++k) *out += g_devs[k].camera_traced;      // the whole job, like ArtStats::rays
  return 0;
}

static int set_option_one(const std::string& n, int64_t value) {
  if (n == "trace_kernel") { if (value != TRACE_COOP && value != TRACE_SIMPLE) return fail("trace_kernel: 0 (cooperative) or 1 (simple)"); g_ctx.opt.trace_kernel = (int)value; }
  else if (n == "queue_segments") { if (value != 1 && value != 2 && value != 4 && value != 8) return fail("queue_segments: 1, 2, 4 or 8"); g_ctx.opt.queue_segments = (int)value; }
  else if (n == "batch_paths") { if (value < 1024 || value > (1ll << 27)) return fail("batch_paths: 1024..2^27 (2 rays per path slot; the trace kernel addresses a ray's 16-byte hit record by a 32-bit byte offset)"); g_ctx.opt.batch_paths = value; g_ctx.trial.reset(); }
  else if (n == "paths_spread") { if (value < -1 || value > 65536) return fail("paths_spread: chunk size in MB, 0 = off (plain hipMalloc), -1 = automatic"); g_ctx.opt.paths_spread_mb = (int)value; release_paths(g_ctx); }
  else if (n == "spread_fail_at") { g_ctx.spread_fail_at = (int)value; release_paths(g_ctx); }      // test option: creating chunk number `value` of the path state fails (-1: never)
  else if (n == "inject_lost") { g_ctx.inject_lost = value != 0; }      // test option: the next pass counts one lost path in its first batch
  else if (n == "blocks_per_cu") { g_ctx.opt.opt_blocks_per_cu = (int)value; g_ctx.blocks_per_cu = 0; }
  else if (n == "query_slice") { if (value < 1 || value > (1ll << 28)) return fail("query_slice: 1 .. 2^28 rays per slice of a device query"); g_ctx.opt.query_slice = value; }
  else if (n == "count_tests") { g_ctx.opt.count_tests = value != 0; }
  else if (n == "camera_dedup") { if (value != 0 && value != 1) return fail("camera_dedup: 0 (every sample's camera ray is traced) or 1 (each distinct camera ray once per batch)"); g_ctx.opt.camera_dedup = value != 0; }
  else if (n == "camera_order") { if (value != 0 && value != 1) return fail("camera_order: 0 (bounce 0 visits the path slots in slot order) or 1 (tile-major: all samples of a 1024-pixel block before the next block)"); g_ctx.opt.camera_order = (int)value; }
  else if (n == "shadow_anyhit") { g_ctx.opt.shadow_anyhit = value != 0; }
  else if (n == "skip_null_shadow") { g_ctx.opt.skip_null_shadow = value != 0; }
  else if (n == "inst_coop") { g_ctx.opt.inst_coop = value != 0; }
  else if (n == "shade_per") { if (value != 0 && value != 2 && value != 4) return fail("shade_per: 0 (measured), 2 or 4"); g_ctx.opt.opt_shade_per = (int)value; }
  else if (n == "ray_chunk") { if (value < 16 || value > 4096 || (value & 15)) return fail("ray_chunk: a multiple of 16, 16..4096"); g_ctx.opt.ray_chunk = (int)value; }
  else if (n == "refill_min") { if (value < 1 || value > 8) return fail("refill_min: 1..8"); g_ctx.opt.refill_min = (int)value; }
  else if (n == "node_min") { if (value < 0 || value > 8) return fail("node_min: 1..8, 0 = automatic"); g_ctx.opt.node_min = (int)value; }
  else if (n == "bvh_width") { if (value != 4 && value != 8) return fail("bvh_width: 4 or 8"); g_ctx.opt.bvh_params.width = (int)value; }
  else if (n == "lds_stack_cap") { if (value < 0 || value > kStackEntries) return fail("lds_stack_cap: 0 (automatic) .. 160"); g_ctx.opt.lds_stack_cap = (int)value; }
  else if (n == "bvh_max_leaf") { if (value < 0 || value > kMaxLeafTris) return fail("bvh_max_leaf: 1..8, 0 = defaults"); g_ctx.opt.bvh_params.max_leaf = value ? (int)value : BvhBuildParams().max_leaf; g_ctx.opt.bvh_params.gpu_max_leaf = (int)value; }
  else if (n == "inst_open") { if (value < 0 || value > 4096) return fail("inst_open: 1 .. 4096 entry points per instance, 0 = chosen from the instances' overlap"); g_ctx.opt.bvh_params.inst_open = (int)value; }
  else if (n == "bvh_spatial_splits") { g_ctx.opt.bvh_params.spatial_alpha = value ? 1.0e-5f : -1.0f; }   // host builder: SBVH reference splitting
  else if (n == "bvh_builder") { if (value < 0 || value > 3) return fail("bvh_builder: 0 host SAH, 1 GPU LBVH, 2 GPU PLOC, 3 GPU SAH"); g_ctx.opt.bvh_params.builder = (int)value; }
  else if (n == "bvh_ploc_radius") { if (value < 1 || value > 64) return fail("bvh_ploc_radius: 1..64"); g_ctx.opt.bvh_params.ploc_radius = (int)value; }
  else if (n == "bvh_leaf_base_milli") { g_ctx.opt.bvh_params.leaf_base = (float)value / 1000.0f; }
  else if (n == "bvh_tri_cost_milli") { g_ctx.opt.bvh_params.tri_cost = (float)value / 1000.0f; }
  else if (n == "bvh_node_cost_milli") { g_ctx.opt.bvh_params.node_cost = (float)value / 1000.0f; }
  else return fail("unknown option " + n);
  return 0;
}
int art_set_option(const char* name, int64_t value) {      // applies to every device of the process
  std::lock_guard<std::mutex> lk(g_mu);
  if (!name) return fail("null option");
  const std::string n(name);
  return each_device(/*stop_at_failure=*/true, [&](int) { return set_option_one(n, value); }, /*switch_gpu=*/false);
}

const char* art_last_error(void) { t_err = g_err; return t_err.c_str(); }

void art_shutdown(void) { std::lock_guard<std::mutex> lk(g_mu); shutdown(); }

}  // extern "C"
