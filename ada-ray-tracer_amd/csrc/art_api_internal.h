// art_api_internal.h -- process-wide backend state (the reference keeps the same kind of singleton:
// g_data in embree_connect.cpp:12-22 and the package-level variables of ray_tracer.ads:20-33,106-109).
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/art_hip.h"
#include "art_event_pairs.h"
#include "art_host_scene.h"
#include "art_move.h"
#include "art_trace.h"
#include "art_pass_plan.h"

namespace art {

constexpr int kMaxDevices = 16;       // art_init_devices: GPUs one process may drive (an MI355X node has 8)
constexpr int kCursorInts = 32 * 9;   // d_cursor: 3 scalars + one work cursor per queue segment, each on its own 128-byte line
constexpr size_t kRecSlack = 4096;    // records past the last one the trace kernel's chunk prefetch may touch

struct DevBuf {
  void* p = nullptr; size_t bytes = 0;
  // option paths_spread: the buffer is a reserved address range backed by separately created physical chunks (HIP virtual memory management)
  std::vector<hipMemGenericAllocationHandle_t> chunks; size_t chunk_bytes = 0, reserved = 0;
  void release();
};
// b = `bytes` of device memory as one address range over separately created chunks (release() is its inverse); fail_at: test option spread_fail_at
hipError_t alloc_spread(DevBuf& b, size_t bytes, size_t chunk, int device, int fail_at = -1);

// What every kind of device-side scene update (art_update.cpp) keeps per context besides its own plan.
struct UpdateLane {
  EventPairs pairs;                                  // event pairs around this context's update kernels
  hipEvent_t ready_ev = nullptr, done_ev = nullptr;  // device 0: the caller's data is ready (contexts k > 0 wait for it); k > 0: this context's update is done
  DevBuf b_stage;                                    // contexts k > 0: peer copy of the caller's data
  bool unread = false;                               // an update was enqueued whose counters no fold has read yet
  uint64_t bad_last = 0; bool bad_reported = true;   // bad items (vertices, matrices) of the last update read; a synchronize reported them (or there were none)
};

// What art_set_option sets and art_init_devices hands to every context (derived state -- blocks_per_cu, trial, paths_are_spread -- is Ctx's).
struct Options {
  int trace_kernel = TRACE_COOP;
  int64_t batch_paths = 128ll << 20;  // path slots per batch (328 B each at depth 8 -> up to 44 GB of the 288 GB HBM; buffers are sized to the frame,
                                      // so a small render takes less): big batches keep late bounces wide (8M -> 32M: +7 %, -> 128M: +1.7 %)
  int opt_blocks_per_cu = 0;
  bool count_tests = false;
  bool camera_dedup = true;      // each distinct camera ray of a batch is generated and traced once (DevPaths::cam_dedup); false: once per sample
  int camera_order = 1;          // the order in which bounce 0 visits a batch's slots (and every later stage its items): 0 slot order (sample-major), 1 tile-major -- all samples
                                 // of 1024 pixels before the next 1024 (art_camera_order.h).  The frame does not depend on it.  Measured: profiles/camera_order/README.md
  int node_min = 0;              // the trace kernel leaves its node loop when fewer than 8 x node_min lanes still expand nodes.  0: 4 (the optimum on C4, profiles/r2_sensitivity.json);
                                 // 2 for an instanced scene -- its groups also wait for instance entries, and leaving the loop for them less often is worth 6 % on I64 (profiles/r5_inst_sweep.py)
  int refill_min = 2;            // idle ray groups of a wave take new rays when two of them are idle (1: at once; measured 0.5-1 % slower)
  int queue_segments = 8;       // the live-ray queue is cut into this many contiguous segments, one per XCD (1 = a single cursor)
  int ray_chunk = 48;            // trace records a wave claims per atomic (and prefetches): 16 -> 48 is worth 1 % on C4, 4 % on C3, 10 % on C5 (the claim stalls the wave)
  bool shadow_anyhit = true;   // shadow rays use the visibility rule instead of a full closest-hit search (same decision)
  bool skip_null_shadow = false;   // DevFrame::skip_null_shadow: true: shadow rays that cannot change the picture are neither traced nor counted (fewer rays than the reference
                                   // issues: off by default).  false: the record schedule still answers them without a walk, and counts them as the reference issues them (make_frame)
  bool inst_coop = true;       // instanced scenes: the cooperative kernel crosses the instance boundary (k_trace_coop<.., INST>); false: k_trace_inst, one ray per lane (A/B, cross-check)
  // Items per thread of k_shade_compact (256 x per items and one global atomic per workgroup): 4 or 2.  Neither wins everywhere (inside one
  // process 2 is 5 % faster on C4, 3 % slower on C5, equal on S4: profiles/r6_shade/trial_check_*.txt; round 5's "+7 % / -10 %" of ab12 were
  // mostly the mapping of the path state, which differed between its processes), so by default the library MEASURES -- without ever
  // waiting for the GPU (round 6; until round 5 the trial blocked the host twice per trial batch, which serialised the devices of a
  // multi-GPU process during their first two batches): after a scene upload or a resize batch 0 runs warm and unmeasured (code-object load,
  // first touch of the path state), batch 1 with 4 items per thread, batch 2 with 2 -- their shade launches' event pairs carry the trial's
  // tag -- and every batch after that with 4 until a synchronize (art_synchronize, art_get_stats, a download: calls that wait anyway) has
  // read both trials' events; then the faster setting is kept.  Two trials only count when their batches had the same number of paths.
  // The picture does not depend on it (the order of the items of a bank carries no meaning).  Option shade_per: 0 automatic, 2, 4.
  int opt_shade_per = 0;
  int lds_stack_cap = 0;        // force the LDS stack size (tests of the overflow path)
  // HOW THE PATH STATE IS MAPPED decides the shade stage's rate (round 6, profiles/r6_bimodal).  The stage runs about forty concurrent streams
  // through the 35-74 GB of path state.  As ONE hipMalloc it took 10.4 or 12.1 ms per batch on C3 (31.7 / 35.9 on C4, 22.2 / 26.0 on C5, 28.0 /
  // 32.5 on S4) depending on the PROCESS -- same binary, same device addresses, same instructions, L2 hits, misses and fabric requests, 16 %
  // more L1 -> L2 read latency -- and 15.0 as physically contiguous memory: the larger the pieces the driver maps the range in, the slower.
  // paths_spread_mb: the path state as one address range over separately created physical chunks of that many MB (HIP virtual memory
  // management, art_api.cpp alloc_spread): the fast mode in every process measured, 13-17 ms to set up, no extra memory; any failure falls
  // back to hipMalloc.  -1 (default): 64 MB chunks when the path state is 1 GB or more; 0: plain hipMalloc; n > 0: n MB chunks always.
  int paths_spread_mb = -1;
  int64_t query_slice = 1ll << 24;             // rays per slice of a query (112 B of scratch per ray: 1.9 GB at 2^24)
  BvhBuildParams bvh_params;
};

enum Counter {           // the words of Ctx::d_counters, which the kernels bump through pointers the host hands them
  CNT_RAYS = 0,          // queries issued by raygen and the shade stages (ArtStats::rays: the reference's Find_Closest_Hit / Compute_Shadow calls, walked or not)
  CNT_STATS = 3, CNT_TRACED = 7,      // [3..7]: box tests, triangle tests, node visits, leaf visits, rays of counting traces (TraceArgs::stats) | the last of them
  CNT_NODE_ITERS = 8, CNT_LEAF_ITERS = 9, CNT_WAVE_ITERS = 10, CNT_LOST = 15, kCounters = 16      // the cooperative kernel's phase counters | paths lost by the wavefront stages (must stay 0)
};

struct Ctx {
  int device = -1; bool device_ready = false; int num_cus = 0; int lds_per_cu = 160 * 1024; std::string arch;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;            // multi-device mode: the stream this context created (stream == own_stream)
  // scene
  bool scene_ready = false;
  HostScene host_scene;
  DevScene scene;
  DevScene* d_scene = nullptr;                 // the same header in HBM (the trace kernels take it by pointer)
  DevBuf b_spheres, b_sphere_mat, b_lights, b_materials, b_bf_pos, b_bf_nrm, b_bf_uv, b_bf_idx, b_nodes, b_qnodes, b_tris, b_qtris, b_m_shade;
  int bvh_stack_bound = 8;      // worst-case traversal stack of the uploaded tree
  // frame
  int width = 0, height = 0, spp = 0;
  int rank = 0, nranks = 1, tile = 32, npix_local = 0;
  DevBuf b_inst, b_tlas_nodes, b_tlas_tris, b_blas_nodes, b_blas_tris;      // instanced scene (DevScene::n_inst > 0)
  DevBuf b_accum, b_screen, b_stage, b_pixmap, b_paths, b_rays, b_ids, b_queue, b_ovf;
  DevBuf b_query;                              // device-resident ray queries: SoA rays + shadow minima + hit records of one slice, and a counter sink
  DevBuf b_denoise;                            // art_denoise_device: its working images, guide records and depth gradients (art_denoise.h)
  DevBuf b_select, b_masklist;                 // mask compaction (art_select.hip): a count word (256 B) + one word per 256 list entries | the masked pass's pixel list, or the iota keys of art_radiance_rays_device; both only grow, like b_pixmap
  hipEvent_t q_ev[2] = {nullptr, nullptr};     // ... their ordering with the context stream when they run on another stream (library -> query, query -> library)
  // art_refit_device (art_refit.hip): the plan is built on the first refit after an upload (the upload drops it); per context, because
  // the GPU builders may number the nodes differently on every device
  struct RefitPlan {
    bool ready = false;
    DevBuf b_idx, b_levels, b_tight, b_bad;            // index triples | node ids level by level, root first | tight box per node (24 B) | bad-vertex counters
    std::vector<int> level_off;                        // level L: b_levels[level_off[L] .. level_off[L + 1])
    uint64_t bad_total = 0;                            // bad vertices since the upload
    UpdateLane lane;                                   // (b_stage: peer copy of pos (+ nrm))
  } refit;
  // art_move_instances_device and art_refit_mesh_device (art_move.hip) share one plan: built by whichever of the two is called first
  // after an upload (the upload drops it), before anything is changed, from the host's copy of the build -- which a mesh refit then leaves
  // stale, so the plan is never built again before the next upload
  struct MovePlan {
    bool ready = false;
    DevBuf b_plan, b_work;                             // MovePlanHost's constant arrays and the meshes' index triples, one after the other | what the kernels write (MoveArgs)
    DevBuf b_tlas;                                     // after art_rebuild_instance_tree_device: the plan's parts that follow the instance tree (its levels, proxy_rec, mesh_base, the tlas_tight scratch); args and levels point into it
    DevBuf b_blas;                                     // after art_rebuild_mesh_tree_device: the plan's parts that follow the meshes' node layout (mesh_base, blas_levels, node_mesh, blas_tight); args and blas_levels point into it
    int32_t n_tlas = 0;                                // nodes of the instance tree the plan works against
    MoveArgs args = MoveArgs();                        // everything but m12f, m_cur_out, bad_total and repads: the call sets those
    std::vector<int> level_off; const int32_t* levels = nullptr;   // the instance tree's level L: levels[level_off[L] .. level_off[L + 1])
    bool small_entries = false;                        // few records per entry point: one wave each (launch_move_entry_boxes)
    UpdateLane lane;                                   // the moves' (b_stage: peer copy of the matrices)
    // per mesh of ArtSceneDesc::meshes, for a mesh refit: its slices of the records (tri_base < 0: no instance shows it), its index triples
    // in HBM, and its tree's levels [level_first, level_end) of blas_level_off
    struct Mesh { int32_t tri_base = -1, n_recs = 0, shade_base = 0, n_prims = 0; int64_t nverts = 0; const int32_t* idx = nullptr; int level_first = 0, level_end = 0; };
    std::vector<Mesh> meshes;
    std::vector<int> blas_level_off; const int32_t* blas_levels = nullptr;   // level k of the meshes' trees: blas_levels[blas_level_off[k] .. blas_level_off[k + 1]), nodes of blas_nodes
    UpdateLane refit_lane;                             // the mesh refits' (b_stage: peer copy of pos (+ nrm))
  } move;
  int* d_live = nullptr;                       // item counts per level: d_live[32 k] = items of bounce k's input set (k >= 1); the dense fold walks them again
  DevBuf b_reduced;                            // device 0, multi-device mode: sum of every device's accum (the RCCL reduce target)
  float* ext_accum = nullptr;
  float* ext_moments = nullptr;                // art_bind_moments: float2 {S1, S2} per pixel, row-major; nullptr: no moments (k_accumulate runs as ever)
  // the rank's pixel list on its way to b_pixmap (build_shard): a pinned copy, and the event behind its last stream-ordered upload
  uint32_t* pixmap_host = nullptr; size_t pixmap_host_bytes = 0; hipEvent_t pixmap_copied = nullptr;
  // work distribution / counters
  int* d_cursor = nullptr;
  unsigned long long* d_counters = nullptr;   // kCounters words, named by enum Counter
  uint64_t camera_traced = 0;     // camera rays the render passes generated and traced since art_resize (art_get_camera_rays_traced; host-side count)
  Options opt; int blocks_per_cu = 0;
  ShadeTrial trial;              // the items-per-thread trial of the shade stage (Options::opt_shade_per, art_pass_plan.h)
  uint64_t lost_reported = 0;    // lost paths (d_counters[CNT_LOST], cumulative) already reported by a synchronize: only synchronize_one advances it
  // the two test options stay outside Options: art_init_devices has never carried them over to the contexts it creates
  int inject_lost = 0;           // test option: the next render pass bumps the self-check counter once in its first batch (tests/test_gpu_parity.py)
  int spread_fail_at = -1; bool paths_are_spread = false;      // test option: the creation of this chunk is made to fail, so that the undo + hipMalloc fallback runs (tests/test_gpu_parity.py) | the path state is a spread mapping (Options::paths_spread_mb)
  // multi-device mode: host clock (steady_clock, ms since the process' first use) at which this device's stream reached the start / the end
  // of its passes -- hipLaunchHostFunc on the stream, so the devices' times share one clock (events of different devices cannot be compared)
  struct PassClock { double t0 = 0.0, t1 = 0.0; };
  std::vector<PassClock*> pass_clock;      // one per pass since the last art_get_reduce_info / resize (heap cells: the callbacks write into them)
  double busy_ms = 0.0, idle_ms = 0.0, start_skew_ms = 0.0;   // folded by art_get_reduce_info
  // timing
  EventPairs stage_pairs;                      // around groups of launches; tag: 0 trace kernel, 1 shade stage, 2 raygen, 3 fold group (art_get_stage_stats) | trial (1 / 2: A / B of the items-per-thread trial) << 4 | the trial's generation << 6
  ArtStageStats stage = ArtStageStats();
  unsigned long long* d_items = nullptr;       // cumulative items_in[16] | items_out[16] (k_acc_items at the end of every batch)
  EventPairs pass_pairs, rebuild_pairs;        // around every render pass (ArtStats::pass_ms) | around the gather of art_rebuild_device
  ArtStats stats = ArtStats();
};

// One context per GPU.  A single-GPU process only ever uses g_devs[0]; art_init_devices(n) fills n of them.  Every entry point holds
// g_mu, so "the current context" is a plain global that the multi-device loops repoint.
extern Ctx g_devs[kMaxDevices];
extern int g_ndev;
extern Ctx* g_cur;
#define g_ctx (*::art::g_cur)
extern std::mutex g_mu;

int fail(const std::string& msg);

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) return ::art::fail(std::string(#expr) + ": " + hipGetErrorString(_e));   \
  } while (0)

int use_dev(int k);                   // make device k's context the current one (g_ctx) and its GPU the current HIP device
struct Dev0Guard { ~Dev0Guard() { g_cur = &g_devs[0]; if (g_devs[0].device >= 0) (void)hipSetDevice(g_devs[0].device); } };   // multi-device loops leave device 0 current on every exit path
// f(k) with context k current, for every context of the process; 1 if any f(k) (or the switch to its GPU) failed.  stop_at_failure: the
// contexts after a failure are not visited.  switch_gpu: context k's GPU is made current too, and device 0 is left current; false (f makes
// no HIP call): only g_cur is repointed, and put back.
template <class F>
int each_device(bool stop_at_failure, F&& f, bool switch_gpu = true) {
  Ctx* const saved = g_cur;
  int rc = 0;
  for (int k = 0; k < g_ndev && !(rc && stop_at_failure); ++k) {
    if (!switch_gpu) g_cur = &g_devs[k];
    if ((switch_gpu && use_dev(k)) || f(k)) rc = 1;
  }
  if (switch_gpu) { Dev0Guard leave_device_0_current; } else g_cur = saved;
  return rc;
}
int ensure(DevBuf& b, size_t bytes);
template <typename T>
int upload(DevBuf& b, const std::vector<T>& v) {
  b.release();
  if (v.empty()) return 0;
  HIP_TRY(hipMalloc(&b.p, v.size() * sizeof(T)));
  b.bytes = v.size() * sizeof(T);
  HIP_TRY(hipMemcpy(b.p, v.data(), b.bytes, hipMemcpyHostToDevice));
  return 0;
}
int check_tree_limits(int width, int64_t n_nodes, int64_t n_tris, bool flat, bool gpu_built, bool have_qnodes, int stack);
struct GpuBvh;
void free_tree(GpuBvh& g);                                             // a built tree nobody adopted (current device: the tree's)
void adopt_tree(Ctx& c, GpuBvh& g, int width);                         // c's b_nodes / b_qnodes / b_tris become g's arrays (g gives them up)
int pad_tri_records(DevBuf& dst, const float* tris, int n, hipStream_t s);   // dst = the 64-byte padded copy of n triangle records, enqueued on s
// ---- device-side scene updates (art_update.cpp) ----
// The stream a caller names (nullptr: the context stream; HIP's legacy handle: the null stream).  Where it is another stream, enter()
// makes it wait for what the context stream holds and leave() makes the context stream wait for it.
struct StreamOrder {
  Ctx& c; hipStream_t cs, qs;
  StreamOrder(Ctx& ctx, hipStream_t st);
  bool other() const { return qs != cs; }
  int enter(), leave();               // (leave() on every way out past enter(), also after a failed launch)
};
void release_updates(Ctx& c);         // the plans go with the scene (upload, rebuild); their events are kept for the next plan
void destroy_updates(Ctx& c);         // shutdown
void reset_update_info();             // the figures are cumulative since the last upload
int sync_updates();                   // art_synchronize, current context, stream idle: fold the event pairs and counters, report a bad update once
// ---- what the device-resident entries share (art_device_entries.cpp) ----
// A caller's plane: device memory of the current context's GPU that holds `bytes` from p on.  check_planes reports the first of a list
// that is not; a null p is skipped (a required plane is refused as null before its list is checked).
struct DevPlane { const void* p; size_t bytes; const char* what; };
int check_planes(std::initializer_list<DevPlane> planes);
// Scratch an entry wants at least this large (buf null: an unused place).  grow_idle allocates what is too small, after waiting for the
// context stream and, where it is another, the caller's: nothing enqueued may still use the old buffer.
struct Grow { DevBuf* buf = nullptr; size_t bytes = 0; };
using GrowList = std::array<Grow, 3>;
int grow_idle(const StreamOrder& order, const GrowList& want);
int end_ordered(StreamOrder& order, const char* name, int rc);      // rc, else the failed launch under the entry's name; then leave()
// One call in the caller's stream order, after the entry's refusals: grow while idle, enter(), body(qs) enqueues on qs and returns rc, the
// launch check, leave() -- also after a failed body.
template <class Body>
int ordered_call(const char* name, hipStream_t st, const GrowList& grow, Body&& body) {
  StreamOrder order(g_ctx, st);
  if (grow_idle(order, grow) || order.enter()) return 1;
  return end_ordered(order, name, body(order.qs));
}
// ---- contexts, scene, frame (art_api.cpp) ----
int ensure_device();
int upload_scene(const ArtSceneDesc* d);
int resize(int w, int h);
int build_shard();                    // the current context's pixel list (rank, nranks, tile) -> b_pixmap, stream-ordered
inline float* accum_ptr() { return g_ctx.ext_accum ? g_ctx.ext_accum : (float*)g_ctx.b_accum.p; }
int download_from(const float* acc_dev, float* accum_host, uint32_t* screen_host, int layout, int spp);
int synchronize_one();                // the current context: wait for its stream, fold its event pairs and counters, report lost paths
int synchronize();                    // every context: synchronize_one, then device 0's reduce events
extern const bool g_debug_addr;       // ART_DEBUG_ADDR is set: device addresses of the path state and the shade trial's verdict on stderr
extern bool g_multi_api;              // the process came up through art_init_devices: passes carry host-clock marks (Ctx::PassClock)
void clock_cb(void* p);               // hipLaunchHostFunc: *(double*)p = the host clock, ms
// ---- the render-pass driver (art_render.cpp) ----
void release_paths(Ctx& c);           // the only way the path state is released
void stack_plan(int& entries, bool& overflow);      // LDS stack entries per ray of a trace launch | rays that go deeper are finished by k_trace_overflow
// One trace launch.  records != nullptr: the bank's rays are already trace records in item order (DevPaths::rec, written by the stage
// that emitted them): no k_analytic pass, the queue is the record array itself.
struct RecordQueue { int fixed; const int* items; int mul; };
// What a trace launch runs on and with.  The render passes and the debug pass take the first three from the context; the
// ray queries name their own, so nothing ever has to change the context for the length of a call.
struct TraceLaunch {
  hipStream_t stream; int kernel; bool count_tests;      // kernel: TRACE_COOP or TRACE_SIMPLE
  bool timed = true;                                     // an event pair (tag 0) around the trace kernel
  const int* item_count = nullptr;
  const RecordQueue* records = nullptr;
  unsigned long long* live_rays = nullptr;               // where the launch counts the rays it issued (nullptr: d_counters[CNT_RAYS], ArtStats::rays)
};
int trace(const DevPaths& q, int n_rays, const TraceLaunch& t);
int check_pass(const ArtPassParams* p);
void make_frame(const ArtPassParams* p, DevFrame& f);
int render_pass_device(const ArtPassParams* p, int32_t* spp_inout);
int compact_mask_device(const uint8_t* mask1b, uint32_t* pixels_out, int64_t cap, uint32_t* count_out, hipStream_t st);
int render_pass_masked(const ArtPassParams* p, const uint8_t* mask1b, uint32_t* counts1u, int32_t* spp_inout, int64_t* pixels_out);   // single device (the caller checked), no synchronize
int radiance_rays(const ArtRadianceParams* p, const float* origins3f, const float* dirs3f, const uint32_t* keys1u, int64_t n, float* radiance3f, float* moments2f);   // single device (the caller checked), no synchronize
int adaptive_estimate_device(const ArtAdaptiveParams* p, const float* accum3f, const float* moments2f, const uint32_t* counts1u, float* mean3f, float* variance1f,
                             float* error1f, uint8_t* mask1b, hipStream_t st);
int svgf_spatial_variance_device(const ArtSvgfSpatialParams* p, const void* hist, const float* variance_in1f, float* variance_out1f, hipStream_t st);
int auto_exposure_device(const ArtExposureParams* p, const float* color3f, void* state, hipStream_t st);
int display_device(const ArtDisplayParams* p, const float* color3f, const void* exposure_state, uint32_t* screen1u, float* ldr3f, hipStream_t st);
int upsample_device(const ArtUpsampleParams* p, const float* lo_color3f, const ArtUpsampleGuides* lo, const ArtUpsampleGuides* hi, float* out3f, uint8_t* fallback1b, hipStream_t st);
int temporal_upsample_device(const ArtTemporalUpsampleParams* p, const float* lo_color3f, const float* lo_moments2f, const ArtTemporalUpsampleGuides* lo,
                             const ArtTemporalUpsampleGuides* hi, const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out,
                             uint8_t* fallback1b, hipStream_t st);
int bloom_device(const ArtBloomParams* p, const float* color3f, const void* exposure_state, float* out3f, float* bloom3f, hipStream_t st);
int firefly_device(const ArtFireflyParams* p, const float* color3f, const float* moments2f, const int32_t* id, float* out3f, float* moments_out2f, uint8_t* clamped1b, hipStream_t st);
int debug_pass(const ArtPassParams* p, float* accum_host, uint32_t* screen_host, int32_t* prim_index, int32_t* mat_id, int32_t* prim_type);
int trace_rays(const float* origins, const float* dirs, const float* tfar, int64_t n, ArtHit* out, int kernel, ArtStats* st);
int query_rays(const float* o3, const float* d3, const float* tnear, const float* tfar, int64_t n, ArtHit* hits, uint8_t* occluded, int kernel, hipStream_t st);
int render_aovs(const ArtPassParams* p, const ArtAovBuffers* out, hipStream_t st, const ArtMotionSource* src = nullptr, float* motion3f = nullptr);   // motion3f: art_render_aovs_motion_device
int aovs_rays(const ArtAovRaysParams* p, const float* o3, const float* d3, const float* tnear, const float* tfar, int64_t n, const ArtAovRayBuffers* out, hipStream_t st);   // single device (the caller checked)
int camera_rays(const ArtPassParams* p, float* o3, float* d3, hipStream_t st);
int ensure_refit_plan();             // the current context's refit plan exists (art_update.cpp); its b_idx holds the flat mesh's index triples
int denoise_device(const ArtDenoiseParams* p, const float* color3f, const float* albedo3f, const float* normal3f, const float* depth, float* out3f, hipStream_t st);
int denoise_svgf_device(const ArtSvgfParams* p, const float* color3f, const float* moments2f, const float* albedo3f, const float* normal3f, const float* depth,
                        float* out3f, float* variance_out, hipStream_t st, bool variance_plane = false);      // variance_plane: art_denoise_svgf_var_device, moments2f is variance1f
int temporal_device(const ArtTemporalParams* p, const float* color3f, const float* moments2f, const float* normal3f, const float* depth, const int32_t* id,
                    const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out, hipStream_t st,
                    const float* motion3f = nullptr, const char* call = "art_temporal_device");      // motion3f: art_temporal_motion_device
void shutdown();
int refit_device(const float* pos3f, const float* nrm3f, int64_t nverts, hipStream_t st);
int get_refit_info(ArtRefitInfo* out);
int rebuild_device(const float* pos3f, const float* nrm3f, int64_t nverts, hipStream_t st);
int get_rebuild_info(ArtRebuildInfo* out);
int get_tree_cost(ArtTreeCost* out);
int move_instances_device(const float* m12f, int64_t n_instances, hipStream_t st);
int get_move_info(ArtMoveInfo* out);
int set_camera(const float* cam_pos, const float* cam_matrix);
int refit_mesh_device(int32_t mesh, const float* pos3f, const float* nrm3f, int64_t nverts, hipStream_t st);
int get_mesh_refit_info(ArtMeshRefitInfo* out);
int rebuild_instance_tree_device(hipStream_t st);
int get_instance_rebuild_info(ArtInstanceRebuildInfo* out);
int get_instance_tree_cost(ArtTreeCost* out);
int rebuild_mesh_tree_device(int32_t mesh, hipStream_t st);
int get_mesh_rebuild_info(ArtMeshRebuildInfo* out);
int get_mesh_tree_cost(int32_t mesh, ArtTreeCost* out);
int export_two_level(ArtTwoLevelInfo* info, const ArtTwoLevelBuffers* buf);   // device 0's two-level scene as it lies in HBM (caller holds g_mu)
int fetch_host_bvh(std::vector<float>& nodes, std::vector<float>& tris, int& width, int& n_tris);   // device 0's tree as host arrays (caller holds g_mu)

}  // namespace art
