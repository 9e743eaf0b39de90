// art_render.cpp -- the render-pass driver behind art_render_pass and art_debug_hit_pass: the path state (its size, layout and
// allocation), the trace launch every caller of the trace kernels goes through, and the per-batch kernel schedule of a pass
// (art_api.cpp's header comment draws it).  What a pass decides on the host without the GPU -- the batch shape, the shade stage's
// items-per-thread trial -- is art_pass_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "art_api_internal.h"
#include "art_frame.h"
#include "art_radiance.h"
#include "art_select.h"
#include "art_stages.h"

namespace art {

static const bool g_debug_live = getenv("ART_DEBUG_LIVE") != nullptr;   // development aid: work-set sizes per stage on stderr (syncs the stream); read once

// Path arrays for P slots and `depth` fold levels, carved out of one allocation.  Hot state exists in TWO banks: every bounce reads one
// and writes the survivors densely into the other (k_shade_compact); cold state (fold stack, terminal value, per-sample radiance, final
// flags) is indexed by slot.  Hot state per item, record layout (round 3, the cooperative schedule): the trace records of its two rays
// (2 x 64 B; the next stage reads the extension ray from there), their hit records (2 x 16 B), prev pdf, flags, shadow epsilon, pending
// explicit colour, item -> slot map, and the extension ray once more as six SoA words for the next stage: 21 words per bank + 32 words of
// records in one array shared by the banks.  Plain layout (one-ray-per-lane schedule, debug pass): rays as SoA arrays, 29 words.
// (record schedule: 6 ray words, ONE 16-byte hit record + the shadow ray's result word, 7 per-path words)
static size_t hot_stride(size_t P) { return (P + 63) & ~(size_t)63; }
static size_t hot_floats(size_t P, bool rec) { return rec ? (size_t)kHotFields * hot_stride(P) + 64 : (14 + 8 + 7) * P; }
// (the trace records are not double-banked: a bank's records are dead once its rays are traced, and the next stage reads none of them)
// cold state: e (depth + 1 levels: dense fold records keep e_k at level k + 1) and w (depth levels) x 3, child (depth levels), term, rad, final flags
static size_t path_floats(size_t P, int depth, bool rec) { return 2 * hot_floats(P, rec) + (rec ? 32 * P + kRecSlack * 16 + 16 : 0) + (7 * (size_t)depth + 3 + 3 + 3 + 1) * P + 64; }

// Every release of the path state goes through here.  hipFree waits for the device, but unmapping a spread path state (alloc_spread) does
// not, and work queued on the context's stream may still use it.
void release_paths(Ctx& c) {
  if (c.b_paths.reserved) (void)hipStreamSynchronize(c.stream);
  c.b_paths.release();
}
// The path state holds at least `bytes` (0), or none could be had (1, *why = HIP's reason; nothing is reported).  may_spread: a new one
// is mapped as Options::paths_spread_mb says (the render passes); else, and when the mapping fails, it is one hipMalloc.
static int ensure_paths(size_t bytes, bool may_spread, hipError_t* why) {
  Ctx& c = g_ctx;
  DevBuf& b = c.b_paths;
  *why = hipSuccess;
  if (b.p && b.bytes >= bytes) return 0;
  release_paths(c);
  *why = hipErrorOutOfMemory; c.paths_are_spread = false;
  // the default (-1): 64 MB chunks for a path state of a gigabyte or more -- where the mapping granularity decides the stage's rate
  const int chunk_mb = !may_spread ? 0 : c.opt.paths_spread_mb > 0 ? c.opt.paths_spread_mb : (c.opt.paths_spread_mb < 0 && bytes >= ((size_t)1 << 30)) ? 64 : 0;
  if (chunk_mb > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    *why = alloc_spread(b, bytes, (size_t)chunk_mb << 20, c.device, c.spread_fail_at);
    if (g_debug_addr) std::fprintf(stderr, "ART_DEBUG_ADDR alloc_spread %.2f GB in chunks of %d MB: %s, %.1f ms\n", (double)bytes / 1e9, chunk_mb, hipGetErrorString(*why),
                                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (*why == hipSuccess) { c.paths_are_spread = true; return 0; }
    b.p = nullptr; (void)hipGetLastError();
  }
  *why = hipMalloc(&b.p, bytes);
  if (*why == hipSuccess) { b.bytes = bytes; return 0; }
  b.p = nullptr; (void)hipGetLastError();
  return 1;
}

// q[0], q[1]: the two banks (slot_id = their own map); both share the cold arrays.  An identity-layout user takes q[0] with slot_id = nullptr
// and final_flags = flags.
static void carve(DevPaths q[2], int P, int depth, bool rec) {
  float* const f0 = (float*)g_ctx.b_paths.p;
  float* f = f0; const size_t p = (size_t)P;
  auto take = [&](size_t n) { float* r = f; f += n; return r; };
  auto align = [&](size_t floats) { f += (floats - ((size_t)(f - f0) & (floats - 1))) & (floats - 1); };
  Rec4* records = nullptr;
  if (rec) { align(16); records = (Rec4*)take(32 * p + kRecSlack * 16); }       // 64-byte records, ONE array for both banks
  for (int k = 0; k < 2; ++k) {
    DevPaths& b = q[k];
    if (rec) {
      // the bank as ONE block (art_scene.h HotField); the pointer fields name its pieces for the kernels that take them one by one
      b.rec = records;
      align(64);
      const size_t st = hot_stride(p);
      float* const h = take((size_t)kHotFields * st);
      b.hot = h; b.stride = (int32_t)st;
      b.ray_ox = h + HF_OX * st; b.ray_oy = h + HF_OY * st; b.ray_oz = h + HF_OZ * st; b.ray_dx = h + HF_DX * st; b.ray_dy = h + HF_DY * st; b.ray_dz = h + HF_DZ * st;
      b.ray_tfar = nullptr;
      b.hit = (DevHit*)(h + HF_HIT * st); b.sh_t = h + HF_SHT * st;
      b.prev_pdf = h + HF_PDF * st; b.flags = (uint32_t*)(h + HF_FLAGS * st); b.sh_min_t = h + HF_SHMIN * st; b.slot_id = (const uint32_t*)(h + HF_SLOT * st);
      b.cand_r = b.cand_g = b.cand_b = nullptr;                                 // (dense fold records: the pending colour has no hot words)
      b.shadow_rule = g_ctx.opt.shadow_anyhit ? 1 : 0; b.has_bvh = g_ctx.scene.n_tris > 0 ? 1 : 0;
      continue;
    } else {
      b.hot = nullptr; b.stride = 0;
      b.rec = nullptr; b.rec_mode = REC_NONE;
      b.ray_ox = take(2 * p); b.ray_oy = take(2 * p); b.ray_oz = take(2 * p);
      b.ray_dx = take(2 * p); b.ray_dy = take(2 * p); b.ray_dz = take(2 * p); b.ray_tfar = take(2 * p);
    }
    align(4);                                                                   // 16-byte hit records
    b.hit = (DevHit*)take(8 * p); b.sh_t = nullptr;
    b.prev_pdf = take(p); b.flags = (uint32_t*)take(p); b.sh_min_t = take(p);
    b.cand_r = take(p); b.cand_g = take(p); b.cand_b = take(p);
    b.slot_id = (const uint32_t*)take(p);
    b.shadow_rule = g_ctx.opt.shadow_anyhit ? 1 : 0; b.has_bvh = g_ctx.scene.n_tris > 0 ? 1 : 0;
  }
  DevPaths& a = q[0];
  a.e_r = take((depth + 1) * p); a.e_g = take((depth + 1) * p); a.e_b = take((depth + 1) * p);
  a.w_r = take(depth * p); a.w_g = take(depth * p); a.w_b = take(depth * p);
  a.child = (int32_t*)take(depth * p);
  a.cold = rec ? a.e_r : nullptr; a.depth = depth;       // (the seven takes above are consecutive: ONE block, art_scene.h DevPaths::cold)
  a.fold_dense = rec ? 1 : 0;                   // the compacted (record) schedule keeps dense fold records; the plain one folds by slot
  a.synth0 = rec ? 1 : 0;                       // ... and lets bounce 0 recompute the camera ray instead of reading it back (nothing else reads raygen's bank)
  a.term_r = take(p); a.term_g = take(p); a.term_b = take(p);
  a.rad_r = take(p); a.rad_g = take(p); a.rad_b = take(p);
  a.final_flags = (uint32_t*)take(p);
  DevPaths& c = q[1];
  c.e_r = a.e_r; c.e_g = a.e_g; c.e_b = a.e_b; c.w_r = a.w_r; c.w_g = a.w_g; c.w_b = a.w_b;
  c.term_r = a.term_r; c.term_g = a.term_g; c.term_b = a.term_b; c.rad_r = a.rad_r; c.rad_g = a.rad_g; c.rad_b = a.rad_b;
  c.final_flags = a.final_flags; c.child = a.child; c.fold_dense = a.fold_dense; c.synth0 = a.synth0; c.cold = a.cold; c.depth = a.depth;
}

// LDS stack per ray: the tree's worst-case bound if 8 workgroups per CU (8 waves per SIMD) still fit in the CU's 160 KB, else the
// largest size that does; then pushes are checked and the few rays that go deeper are finished by k_trace_overflow.
void stack_plan(int& entries, bool& overflow) {
  Ctx& c = g_ctx;
  const int per_block = c.lds_per_cu / 8, groups = 64 / c.scene.node_width;        // 8 workgroups of 4 waves per CU = 8 waves per SIMD
  int cap = per_block / (4 * groups * 8) - 3;     // entries per ray (+ 2 guard entries + the sink of masked pushes)
  if (c.opt.lds_stack_cap > 0) cap = c.opt.lds_stack_cap;
  cap = std::min(cap, 64 * 1024 / (4 * groups * 8) - 3);      // one workgroup's dynamic LDS stays within the 64 KB a launch may ask for by default
  entries = std::min(c.bvh_stack_bound, cap);
  overflow = c.bvh_stack_bound > entries;
}

static int coop_grid() {
  Ctx& c = g_ctx;
  int entries; bool ovf; stack_plan(entries, ovf);
  if (c.opt.opt_blocks_per_cu > 0) return c.num_cus * c.opt.opt_blocks_per_cu;
  return c.num_cus * trace_coop_blocks_per_cu(entries, c.scene.node_width);
}

static void fill_trace_args(TraceArgs& a, const DevPaths& q, int n_rays) {
  Ctx& c = g_ctx;
  a.n_rays = n_rays; a.width = c.scene.node_width; a.instanced = c.scene.n_inst > 0 ? (c.opt.inst_coop ? 1 : 2) : 0;
  a.inst = c.scene.inst; a.inst_shift = c.scene.inst_shift;
  { int e; bool o; stack_plan(e, o); a.stack_entries = e; a.stack_overflow = o ? 1 : 0; }
  a.node_min = c.opt.node_min ? c.opt.node_min : (c.scene.n_inst > 0 ? 2 : 4); a.refill_min = c.opt.refill_min; a.segments = c.opt.queue_segments; a.chunk = c.opt.ray_chunk;
  a.ray_ox = q.ray_ox; a.ray_oy = q.ray_oy; a.ray_oz = q.ray_oz; a.ray_dx = q.ray_dx; a.ray_dy = q.ray_dy; a.ray_dz = q.ray_dz; a.ray_tfar = q.ray_tfar;
  a.hit = q.hit; a.sh_t = q.sh_t;
  a.nodes = c.scene.nodes; a.qnodes = (const uint32_t*)c.b_qnodes.p; a.tris = c.scene.tris; a.qtris = (const float*)c.b_qtris.p; a.n_tris = c.scene.n_tris;
  a.sh_min = (c.opt.shadow_anyhit && q.sh_min_t && n_rays > q.P) ? q.sh_min_t : nullptr; a.shadow_begin = q.P;
  a.cursor = c.d_cursor; a.stats = c.d_counters + CNT_STATS; a.live_rays = c.d_counters + CNT_RAYS;
  a.queue = (int*)c.b_queue.p; a.queue_count = c.d_cursor + 1;
  a.rec = (float4*)c.b_queue.p;
  a.ovf_queue = (int*)c.b_ovf.p; a.ovf_count = c.d_cursor + 2;
  a.item_count = nullptr;
  a.queue_fixed = -1; a.queue_items = nullptr; a.queue_mul = 1;
}

static TraceLaunch pass_launch() { const Ctx& c = g_ctx; return {c.stream, c.opt.trace_kernel, c.opt.count_tests}; }
// the tag of a stage_pairs pair.  trial: 1 / 2 = a shade launch of the items-per-thread trial A / B (Options::opt_shade_per)
static uint8_t ev_tag(int kind, int trial = 0) { return g_ctx.trial.tag(kind, trial); }

int trace(const DevPaths& q, int n_rays, const TraceLaunch& t) {
  Ctx& c = g_ctx;
  const bool coop = (t.kernel == TRACE_COOP);
  if ((int64_t)n_rays > (1ll << 28)) return fail("internal: more than 2^28 rays in one trace launch (32-bit byte offsets of the 16-byte hit records)");
  if (t.records && !coop) return fail("internal: trace records without the cooperative kernel");
  if (coop && !t.records && ensure(c.b_queue, ((size_t)n_rays + kRecSlack) * kTraceRecBytes)) return 1;      // live-ray queue: one 64-byte trace record per queued ray (+ one chunk of slack for the chunk prefetch)
  TraceArgs a; fill_trace_args(a, q, n_rays);
  a.item_count = t.item_count;
  if (t.live_rays) a.live_rays = t.live_rays;
  if (t.records) { a.rec = (float4*)q.rec; a.queue_fixed = t.records->fixed; a.queue_items = t.records->items; a.queue_mul = t.records->mul; }
  if (coop && a.stack_overflow && ensure(c.b_ovf, (size_t)n_rays * sizeof(int))) return 1;
  a.ovf_queue = (int*)c.b_ovf.p;
  if (coop) HIP_TRY(hipMemsetAsync(c.d_cursor, 0, kCursorInts * sizeof(int), t.stream));
  if (coop && !t.records) launch_analytic(t.stream, c.scene, a, t.count_tests);   // outside the trace-kernel event pair
  EventPairs::Timer timer;
  if (t.timed) HIP_TRY(c.stage_pairs.begin(timer, t.stream, ev_tag(0)));
  // a workgroup keeps 4 waves x (64 / width) rays in flight: a handful of rays (the legacy per-ray seam) gets a handful of workgroups
  const int rays_per_block = 4 * (64 / std::max(1, c.scene.node_width));
  const int grid = (int)std::min<int64_t>(coop_grid(), ((int64_t)n_rays + rays_per_block - 1) / rays_per_block);
  launch_trace(t.stream, c.d_scene, a, t.kernel, t.count_tests, std::max(1, grid));
  HIP_TRY(timer.end());
  HIP_TRY(hipGetLastError());
  return 0;
}

int check_pass(const ArtPassParams* p) {
  Ctx& c = g_ctx;
  if (!p) return fail("null ArtPassParams");
  if (!c.scene_ready) return fail("no scene uploaded (art_upload_scene)");
  if (c.width <= 0) return fail("no viewport (art_resize)");
  if (p->max_depth < 1 || p->max_depth > 16) return fail("max_depth must be 1..16");
  if (p->vthreads < 1) return fail("vthreads must be >= 1");
  if (p->layout != ART_LAYOUT_ADA_XY && p->layout != ART_LAYOUT_ROW_MAJOR) return fail("unknown layout");
  return 0;
}

void make_frame(const ArtPassParams* p, DevFrame& f) {
  Ctx& c = g_ctx;
  f.width = c.width; f.height = c.height;
  f.render_type = p->render_type; f.aa_on = p->aa_on ? 1 : 0; f.max_depth = p->max_depth;
  f.seed_lo = (uint32_t)p->seed; f.seed_hi = (uint32_t)(p->seed >> 32);
  std::memcpy(f.background, p->background, 12);
  const float fov = kHalfPi;                                   // ray_tracer.adb:63  Pi/2.0
  f.cam_z = -(float)c.width / safe_tan(fov / 2.0f);            // ray_tracer.adb:67
  // null shadow rays (DevFrame::skip_null_shadow): the record schedule answers them without a walk and counts them, as it does a camera
  // query that shares its ray; the counting variant and the one-ray-per-lane schedule walk every one of them
  const bool walk_all = c.opt.count_tests || c.opt.trace_kernel != TRACE_COOP;
  f.skip_null_shadow = c.opt.skip_null_shadow ? kNullShadowDropped : (walk_all ? kNullShadowTraced : kNullShadowCounted);
}

// The batch shape of a pass (plan_batch: pc * sc <= batch_paths) and a path state that holds one batch.  The result does not depend on
// the batching (the RNG is keyed by pixel, sample and bounce), so when HBM is short (a shared GPU, a caller holding memory) the batch is
// halved until it fits.  Two buffers belong to a batch: the path state and the live-ray queue (one 64-byte trace record for each of the
// up to 2 rays of a path).
static int plan_and_allocate(const ArtPassParams* p, int npix, int S, int per, BatchPlan& plan) {
  Ctx& c = g_ctx;
  const bool rec_layout = (c.opt.trace_kernel == TRACE_COOP);              // the cooperative schedule keeps its rays as trace records inside the path state
  for (int64_t cap = std::max<int64_t>(c.opt.batch_paths, per);; cap /= 2) {
    plan = plan_batch(npix, S, per, cap);
    const size_t bytes = path_floats((size_t)plan.pc * plan.sc, p->max_depth, rec_layout) * 4 + 256;
    hipError_t e;
    if (!ensure_paths(bytes, /*may_spread=*/true, &e)) break;
    if (g_debug_live) std::fprintf(stderr, "path state: %.2f GB refused (%s)\n", (double)bytes / 1e9, hipGetErrorString(e));
    if (e != hipErrorOutOfMemory || cap <= 65536) return fail(std::string("path buffers: ") + hipGetErrorString(e));
  }
  const int pc = plan.pc, sc = plan.sc;
  if (g_debug_live) std::fprintf(stderr, "path state: %d pixels x %d samples per batch, %.2f GB\n", pc, sc, (double)g_ctx.b_paths.bytes / 1e9);
  if (g_debug_addr) {
    DevPaths bk[2]; std::memset(bk, 0, sizeof bk);
    carve(bk, pc * sc, p->max_depth, rec_layout);
    std::fprintf(stderr, "ART_DEBUG_ADDR spread %d paths %p bytes %zu P %d rec %p hot0 %p hot1 %p stride %d cold %p live %p counters %p cursor %p\n", c.paths_are_spread ? 1 : 0, g_ctx.b_paths.p, g_ctx.b_paths.bytes, pc * sc,
                 (void*)bk[0].rec, (void*)bk[0].hot, (void*)bk[1].hot, bk[0].stride, (void*)bk[0].cold, (void*)c.d_live, (void*)c.d_counters, (void*)c.d_cursor);
  }
  return 0;
}

// One batch of the compacted record schedule.  Compacted work sets: raygen fills bank 0 (one item per slot); stage b shades the items of
// bank b & 1 and writes the survivors densely into the other bank.  d_live[0] / d_live[32]: the banks' item counts.  Every stage leaves
// its rays as trace records in its output bank (round 3), at positions given by the item index; the trace kernel reads them from there
// in item order.  cam_dedup: DevPaths::cam_dedup (0: every slot's camera ray is traced); cam_n: camera rays the batch generates and traces.
// rays != nullptr (art_radiance_rays_device): the two ends of the batch are art_radiance.hip's -- raygen reads the caller's rays, bounce 0 reads
// them from bank 0 (synth0 = 0: the stage's non-camera instantiation), the fold's result goes to the caller's planes -- and the frame's
// counters (ArtStageStats' batches and items) stay as they are.
static int render_batch_records(const ArtPassParams* p, const DevFrame& F, const TraceLaunch& launch, DevPaths bank[2], int sn, int cam_dedup, int cam_n, ShadeTrial::Batch tb,
                                const RayBatch* rays = nullptr) {
  Ctx& c = g_ctx;
  const int trial = tb.trial, shade_per = tb.shade_per;
  if (!c.d_live) HIP_TRY(hipMalloc(&c.d_live, 32 * 18 * sizeof(int)));          // d_live[32 k]: items of level k (the input set of bounce k), k = 1 .. max_depth <= 16
  unsigned long long* const rays_b = c.opt.count_tests ? c.d_counters + CNT_TRACED : nullptr;
  bank[0].rec_mode = REC_EXT;
  DevPaths q = bank[0];                            // identity layout for raygen
  q.slot_id = nullptr;
  q.cam_dedup = cam_dedup;
  DevPaths qgen = q; qgen.P = cam_n;               // raygen's slots: [0, cam_n) are the distinct rays (slot = (sample & 3 within the batch) * pn + pixel)
  if (!c.d_items) { HIP_TRY(hipMalloc(&c.d_items, 32 * sizeof(unsigned long long))); HIP_TRY(hipMemsetAsync(c.d_items, 0, 32 * sizeof(unsigned long long), c.stream)); }
  { EventPairs::Timer t; HIP_TRY(c.stage_pairs.begin(t, c.stream, ev_tag(2)));
    if (rays) launch_raygen_rays(c.stream, c.scene, qgen, *rays); else launch_raygen(c.stream, F, c.scene, qgen); }
  launch_bump(c.stream, c.d_counters + CNT_RAYS, rays_b, (unsigned long long)q.P);      // ArtStats::rays: one camera query per sample (the reference's Find_Closest_Hit calls), however many were traced
  { const RecordQueue rq = {cam_n, nullptr, 1}; TraceLaunch t = launch; t.records = &rq; if (trace(q, cam_n, t)) return 1; }
  for (int b = 0; b < p->max_depth; ++b) {
    const int in = b & 1, out = in ^ 1;
    const DevPaths& qi = (b == 0) ? q : bank[in];
    const bool last = b + 1 >= p->max_depth;
    bank[out].rec_mode = (p->render_type == ART_PT_STUPID) ? REC_EXT : (last ? REC_SHADOW : REC_BOTH);
    int* const n_in = c.d_live + 32 * b; int* const n_out = c.d_live + 32 * (b + 1);      // per level: the fold walks them again
    HIP_TRY(hipMemsetAsync(n_out, 0, sizeof(int), c.stream));
    { EventPairs::Timer t; HIP_TRY(c.stage_pairs.begin(t, c.stream, ev_tag(1, trial)));
      launch_shade_compact(c.stream, F, c.scene, qi, bank[out], b, b == 0 ? nullptr : n_in, n_out,
                           const_cast<uint32_t*>(bank[out].slot_id), c.d_counters + CNT_LOST, c.d_counters + CNT_RAYS, rays_b, shade_per, c.opt.camera_order); }
    if (b == 0 && c.inject_lost) { launch_bump(c.stream, c.d_counters + CNT_LOST, nullptr, 1ull); c.inject_lost = 0; }      // test option: what a stage does when it loses a path
    if (g_debug_live) {
      int n = -1; unsigned long long r0 = 0;
      (void)hipStreamSynchronize(c.stream); (void)hipMemcpy(&n, n_out, 4, hipMemcpyDeviceToHost); (void)hipMemcpy(&r0, c.d_counters + CNT_RAYS, 8, hipMemcpyDeviceToHost);
      std::fprintf(stderr, "stage %d: items out %d of %d, rays so far %llu\n", b, n, q.P, r0);
    }
    if (!last || p->render_type != ART_PT_STUPID) {
      const RecordQueue rq = {-1, n_out, bank[out].rec_mode == REC_BOTH ? 2 : 1};
      TraceLaunch t = launch; t.item_count = n_out; t.records = &rq;
      if (trace(bank[out], 2 * q.P, t)) return 1;
    }
  }
  const int last = p->max_depth & 1;              // the bank the last stage wrote
  EventPairs::Timer fold_timer;
  HIP_TRY(c.stage_pairs.begin(fold_timer, c.stream, ev_tag(3)));
  launch_resolve_last(c.stream, bank[last], c.d_live + 32 * p->max_depth, p->max_depth - 1);
  if (bank[last].fold_dense) launch_fold_levels(c.stream, F, bank[last], p->max_depth, c.d_live);
  else launch_fold(c.stream, F, bank[last]);
  if (rays) launch_accumulate_rays(c.stream, q, sn, *rays);
  else if (c.ext_moments) launch_accumulate_moments(c.stream, F, q, sn, accum_ptr(), c.ext_moments);
  else launch_accumulate(c.stream, F, q, sn, accum_ptr());
  HIP_TRY(fold_timer.end());
  if (rays) return 0;
  launch_acc_items(c.stream, c.d_live, p->max_depth, q.P, c.d_items);
  c.stage.batches += 1;
  return 0;
}

// One batch of the one-ray-per-lane cross-check kernel: the plain schedule over all slots, in place.
static int render_batch_plain(const ArtPassParams* p, const DevFrame& F, const TraceLaunch& launch, const DevPaths& bank0, int sn) {
  Ctx& c = g_ctx;
  DevPaths q = bank0;
  q.slot_id = nullptr;
  q.final_flags = q.flags;
  launch_raygen(c.stream, F, c.scene, q);
  for (int b = 0; b < p->max_depth; ++b) {
    if (trace(q, b == 0 ? q.P : 2 * q.P, launch)) return 1;
    launch_shade(c.stream, F, c.scene, q, b);
  }
  if (p->render_type != ART_PT_STUPID) { if (trace(q, 2 * q.P, launch)) return 1; }
  launch_finish(c.stream, F, q, p->max_depth - 1);
  if (c.ext_moments) launch_accumulate_moments(c.stream, F, q, sn, accum_ptr(), c.ext_moments);
  else launch_accumulate(c.stream, F, q, sn, accum_ptr());
  return 0;
}

// A pixel list a pass walks: the context's own (b_pixmap, npix_local), or the compacted list of a masked pass.
// rays != nullptr (art_radiance_rays_device): the list is the caller's n rays -- `pixels` their RNG keys (nullptr: ray i has key i, which
// only a pass of ONE ray chunk may leave to DevPaths::pixmap's identity), rays->sample_base the sample index of the call's first path
// instead of the frame's spp, the planes those of the call.  Such a pass reads and writes nothing of the frame.
struct RaySource { RayBatch all; uint32_t sample_base; };
struct PixelList { const uint32_t* pixels; int n; bool masked; const RaySource* rays = nullptr; };

// The batch of samples [s0, s0 + sn) of the pixels [px0, px0 + pn) of the pixel list L.
static int render_batch(const ArtPassParams* p, const DevFrame& F, const TraceLaunch& launch, const PixelList& L, int px0, int pn, int s0, int sn) {
  Ctx& c = g_ctx;
  const bool records = (c.opt.trace_kernel == TRACE_COOP);
  DevPaths bank[2]; std::memset(bank, 0, sizeof bank);
  for (DevPaths& b : bank) { b.P = pn * sn; b.npix = pn; b.pixmap = L.pixels ? L.pixels + px0 : nullptr; b.sample_base = (L.rays ? L.rays->sample_base : (uint32_t)c.spp) + (uint32_t)s0; }
  carve(bank, bank[0].P, p->max_depth, records);
  if (L.rays) {                                    // the caller's rays: the record schedule (checked by the entry), nothing synthesised, nothing shared
    for (DevPaths& b : bank) b.synth0 = 0;
    const RayBatch& A = L.rays->all;
    const RayBatch R = {A.origins3f + 3 * (size_t)px0, A.dirs3f + 3 * (size_t)px0, A.radiance3f + 3 * (size_t)px0, A.moments2f ? A.moments2f + 2 * (size_t)px0 : nullptr};
    const ShadeTrial::Batch per = {0, c.opt.opt_shade_per ? c.opt.opt_shade_per : (c.trial.phase >= 4 ? c.trial.per : 4)};      // out of the trial, as a masked pass
    if (render_batch_records(p, F, launch, bank, sn, 0, bank[0].P, per, &R)) return 1;
    HIP_TRY(hipGetLastError());
    return 0;
  }
  // items per thread of the shade stage for this batch: the option, the measured choice, or a trial (art_pass_plan.h ShadeTrial).
  // Nothing here waits for the GPU: a trial batch only tags its shade launches' event pairs, and the next call that synchronises
  // anyway reads them (collect_timing) -- Render_Pass releases all its workers before it waits for any (ray_tracer.adb:271-277).
  // A masked pass stays out of the trial (its batches have sizes of their own): the option, else the decided value, else 4.
  const ShadeTrial::Batch trial = L.masked ? ShadeTrial::Batch{0, c.opt.opt_shade_per ? c.opt.opt_shade_per : (c.trial.phase >= 4 ? c.trial.per : 4)}
                                           : c.trial.next((int64_t)pn * sn, c.opt.opt_shade_per, records);
  // Option camera_dedup: the batch's distinct camera rays -- one per (pixel, sample & 3), DevPaths::cam_dedup -- are generated and traced
  // once; bounce 0 still runs over all P slots and reads every slot's hit from its distinct ray.  The counting variant traces every
  // sample's camera ray: its contract is "equal to the oracle's walk".
  const bool dedup = c.opt.camera_dedup && !c.opt.count_tests && records;
  // U distinct rays per pixel: 4 with AA on (a sample chunk is a whole number of Generate4RayDirections groups: sc and S are multiples of 4), 1 with AA off
  const int cam_u = p->aa_on ? 4 : 1;
  const int cam_n = dedup ? cam_u * pn : bank[0].P;      // camera rays this batch generates and traces
  c.camera_traced += (uint64_t)cam_n;
  if (records ? render_batch_records(p, F, launch, bank, sn, dedup ? cam_u : 0, cam_n, trial) : render_batch_plain(p, F, launch, bank[0], sn)) return 1;
  HIP_TRY(hipGetLastError());
  return 0;
}

// What a render pass refuses on its parameters and the context's state, apart from the spp rule; changes nothing.
static int check_render_pass(const ArtPassParams* p) {
  Ctx& c = g_ctx;
  if (check_pass(p)) return 1;
  if (p->render_type == ART_RT_DEBUG || p->render_type == ART_RT_WHITTED) return fail("debug render types go through art_debug_hit_pass");
  if (p->render_type < ART_PT_STUPID || p->render_type > ART_PT_MIS) return fail("unknown render_type");
  if (c.scene.n_inst > 0 && c.opt.trace_kernel != TRACE_COOP) return fail("an instanced scene renders through the record schedule only (option trace_kernel = 0)");
  return 0;
}
static const char* const kSppRule = "with anti-aliasing on, spp must be a multiple of 4 (Generate4RayDirections order)";

// One Render_Pass of the current context over the pixel list L: check, plan and allocate, then enqueue batch after batch.
// With a ray source (PixelList::rays; its entry, radiance_rays, has made the checks) the pass is the same plan and the same batches, and
// nothing of the frame: spp, ArtStats::samples and pass_ms stay as they are.
static int render_pass_list(const ArtPassParams* p, int32_t* spp_inout, const PixelList& L0) {
  Ctx& c = g_ctx;
  const bool frame = (L0.rays == nullptr);
  if (frame && check_render_pass(p)) return 1;
  const int per = p->aa_on ? 4 : 1;
  if (frame && spp_inout) c.spp = *spp_inout;
  if (frame && p->aa_on && (c.spp % 4) != 0) return fail(kSppRule);
  const int S = p->vthreads * per;           // samples this pass
  const int npix = L0.n;
  DevFrame F; make_frame(p, F);
  BatchPlan plan = {0, 0};
  if (npix > 0 && plan_and_allocate(p, npix, S, per, plan)) return 1;
  PixelList L = L0;
  if (!frame && !L.pixels && npix > 0 && plan.pc < npix) {
    // rays without keys in more than one ray chunk: a chunk past ray 0 needs its keys spelled out (b_masklist: a list scratch of this stream)
    if (grow_idle(StreamOrder(c, nullptr), GrowList{Grow{&c.b_masklist, (size_t)npix * sizeof(uint32_t)}})) return 1;
    launch_iota_keys(c.stream, (uint32_t*)c.b_masklist.p, npix);
    L.pixels = (const uint32_t*)c.b_masklist.p;
  }
  EventPairs::Timer pass_timer;
  if (frame) HIP_TRY(c.pass_pairs.begin(pass_timer, c.stream));
  struct Uncounted { EventPairs::Timer& t; ~Uncounted() { t.cancel(); } } uncounted{pass_timer};      // a pass that fails midway never enters pass_ms
  const TraceLaunch launch = pass_launch();
  Ctx::PassClock* clock = nullptr;
  if (g_multi_api && frame) { clock = new Ctx::PassClock; c.pass_clock.push_back(clock); HIP_TRY(hipLaunchHostFunc(c.stream, clock_cb, &clock->t0)); }
  for (int px0 = 0; px0 < npix; px0 += plan.pc) {
    const int pn = std::min(plan.pc, npix - px0);
    for (int s0 = 0; s0 < S; s0 += plan.sc) {
      if (render_batch(p, F, launch, L, px0, pn, s0, std::min(plan.sc, S - s0))) return 1;
    }
  }
  HIP_TRY(pass_timer.end());
  if (clock) HIP_TRY(hipLaunchHostFunc(c.stream, clock_cb, &clock->t1));
  if (!frame) return 0;
  c.spp += S;
  c.stats.samples += (uint64_t)npix * S;
  if (spp_inout) *spp_inout = c.spp;
  return 0;
}
static int render_pass_one(const ArtPassParams* p, int32_t* spp_inout) {
  Ctx& c = g_ctx;
  return render_pass_list(p, spp_inout, PixelList{(const uint32_t*)c.b_pixmap.p, c.npix_local, false});
}

// ---- mask compaction and the masked pass (art_select.hip) --------------------------------------------------------------------------
// b_select = the count word of the masked pass (its first 256 bytes) | one word per workgroup of 256 list entries
static size_t select_bytes(int n) { return 256 + (size_t)select_blocks(n) * sizeof(uint32_t); }
// the three launches over the context's pixel list (n = npix_local >= 1 entries) on st
static void enqueue_compact(hipStream_t st, const uint8_t* mask1b, uint32_t* pixels_out, uint32_t* count_out) {
  Ctx& c = g_ctx;
  SelectArgs A;
  A.mask = mask1b; A.pixmap = (const uint32_t*)c.b_pixmap.p; A.n = c.npix_local;
  A.block_sums = (uint32_t*)((char*)c.b_select.p + 256); A.out = pixels_out;
  launch_compact_mask(st, A, count_out);
}

int compact_mask_device(const uint8_t* mask1b, uint32_t* pixels_out, int64_t cap, uint32_t* count_out, hipStream_t st) {
  Ctx& c = g_ctx;
  const std::string name = "art_compact_mask_device";
  if (!mask1b || !pixels_out || !count_out) return fail(name + ": null mask1b, pixels_out or count_out");
  if (c.width <= 0) return fail(name + ": no viewport (art_resize)");
  if ((int64_t)c.npix_local > (1ll << 28)) return fail(name + ": the pixel list holds more than 2^28 pixels");
  if (cap < (int64_t)c.npix_local) return fail(name + ": cap " + std::to_string(cap) + " is smaller than the rank's pixel list (" + std::to_string(c.npix_local) + " pixels)");
  if (ensure_device()) return 1;
  if (check_planes({{mask1b, (size_t)c.width * (size_t)c.height, "mask1b"}, {pixels_out, 4 * (size_t)cap, "pixels_out"}, {count_out, 4, "count_out"}})) return 1;
  return ordered_call(name.c_str(), st, GrowList{Grow{c.npix_local > 0 ? &c.b_select : nullptr, select_bytes(c.npix_local)}}, [&](hipStream_t qs) {
    if (c.npix_local > 0) enqueue_compact(qs, mask1b, pixels_out, count_out);
    else if (hipMemsetAsync(count_out, 0, 4, qs) != hipSuccess) return fail(name + ": hipMemsetAsync failed");
    return 0;
  });
}

// art_render_pass_masked on the current context (single device: the caller checked).  Everything is refused before the first launch.
int render_pass_masked(const ArtPassParams* p, const uint8_t* mask1b, uint32_t* counts1u, int32_t* spp_inout, int64_t* pixels_out) {
  Ctx& c = g_ctx;
  const std::string name = "art_render_pass_masked";
  if (check_render_pass(p)) return 1;
  if (p->aa_on && ((spp_inout ? *spp_inout : c.spp) % 4) != 0) return fail(kSppRule);
  if (!mask1b) return fail(name + ": null mask1b");
  if ((int64_t)c.npix_local > (1ll << 28)) return fail(name + ": the pixel list holds more than 2^28 pixels");
  const size_t N = (size_t)c.width * (size_t)c.height;
  if (check_planes({{mask1b, N, "mask1b"}, {counts1u, 4 * N, "counts1u"}})) return 1;
  uint32_t count = 0;
  const uint32_t* list = nullptr;
  if (c.npix_local > 0) {
    if (grow_idle(StreamOrder(c, nullptr), GrowList{Grow{&c.b_select, select_bytes(c.npix_local)}, Grow{&c.b_masklist, (size_t)c.npix_local * sizeof(uint32_t)}})) return 1;
    uint32_t* const d_count = (uint32_t*)c.b_select.p;
    enqueue_compact(c.stream, mask1b, (uint32_t*)c.b_masklist.p, d_count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));               // the one wait: the host plans the batches from the list's length
    if (count > (uint32_t)c.npix_local) return fail(name + ": internal: the compacted list is longer than the pixel list");
    list = (const uint32_t*)c.b_masklist.p;
  }
  if (render_pass_list(p, spp_inout, PixelList{list, (int)count, true})) return 1;
  if (counts1u && count > 0) {
    launch_add_counts(c.stream, list, (int)count, counts1u, (uint32_t)(p->vthreads * (p->aa_on ? 4 : 1)));
    HIP_TRY(hipGetLastError());
  }
  if (pixels_out) *pixels_out = (int64_t)count;
  return 0;
}

// art_radiance_rays_device on the current context (single device: the caller checked).  Every refusal comes before the first launch, and
// those that need no GPU before the device is looked for.  The pass is render_pass_list's over the caller's rays: no anti-aliasing, one
// "virtual thread" per sample, no background.
int radiance_rays(const ArtRadianceParams* p, const float* origins3f, const float* dirs3f, const uint32_t* keys1u, int64_t n, float* radiance3f, float* moments2f) {
  Ctx& c = g_ctx;
  const std::string name = "art_radiance_rays_device";
  if (!p) return fail(name + ": null ArtRadianceParams");
  if (p->render_type == ART_RT_DEBUG || p->render_type == ART_RT_WHITTED) return fail(name + ": debug render types have no radiance (ART_PT_STUPID, ART_PT_SHADOW or ART_PT_MIS)");
  if (p->render_type < ART_PT_STUPID || p->render_type > ART_PT_MIS) return fail(name + ": unknown render_type");
  if (p->max_depth < 1 || p->max_depth > 16) return fail(name + ": max_depth must be 1..16");
  if (p->samples < 1) return fail(name + ": samples must be >= 1");
  if (n < 0 || n > (1ll << 28)) return fail(name + ": n must be 0 .. 2^28");
  if (n == 0) return 0;
  if (!origins3f || !dirs3f || !radiance3f) return fail(name + ": null origins3f, dirs3f or radiance3f");
  if (!c.scene_ready) return fail(name + ": no scene uploaded (art_upload_scene)");
  if (c.opt.trace_kernel != TRACE_COOP) return fail(name + ": the cooperative record schedule only (option trace_kernel = 0)");
  if (ensure_device()) return 1;
  const size_t N = (size_t)n;
  if (check_planes({{origins3f, 12 * N, "origins3f"}, {dirs3f, 12 * N, "dirs3f"}, {keys1u, 4 * N, "keys1u"}, {radiance3f, 12 * N, "radiance3f"}, {moments2f, 8 * N, "moments2f"}})) return 1;
  ArtPassParams pp = ArtPassParams();      // (background: zero, and never read without anti-aliasing)
  pp.render_type = p->render_type; pp.aa_on = 0; pp.max_depth = p->max_depth; pp.vthreads = p->samples; pp.seed = p->seed; pp.layout = ART_LAYOUT_ROW_MAJOR;
  const RaySource src = {RayBatch{origins3f, dirs3f, radiance3f, moments2f}, p->sample_base};
  return render_pass_list(&pp, nullptr, PixelList{keys1u, (int)n, true, &src});
}

// One Render_Pass on every device of the process: each GPU renders the pixel tiles it owns into its own accum buffer, asynchronously on
// its own stream (the host only enqueues: ~100 calls per device and pass).  The buffers meet in reduce_accum() when somebody asks
// for the image.  What the caller gets back is device 0's spp.
int render_pass_device(const ArtPassParams* p, int32_t* spp_inout) {
  int32_t spp_out = spp_inout ? *spp_inout : 0;
  const int rc = each_device(/*stop_at_failure=*/true, [&](int k) {
    int32_t spp_k = spp_inout ? *spp_inout : 0;
    if (render_pass_one(p, spp_inout ? &spp_k : nullptr)) return 1;
    if (k == 0) spp_out = spp_k;
    return 0;
  });
  if (rc) return 1;
  if (spp_inout) *spp_inout = spp_out;
  return 0;
}

static int debug_pass_one(const ArtPassParams* p, float* accum_host, uint32_t* screen_host, int32_t* prim_index, int32_t* mat_id, int32_t* prim_type) {
  Ctx& c = g_ctx;
  if (check_pass(p)) return 1;
  ArtPassParams pp = *p; pp.aa_on = 0;
  DevFrame F; make_frame(&pp, F);
  const int npix = c.npix_local; const size_t n = (size_t)c.width * c.height;
  if (ensure(c.b_ids, n * 12)) return 1;
  HIP_TRY(hipMemsetAsync(c.b_ids.p, 0xff, n * 12, c.stream));
  int32_t* d_pi = (int32_t*)c.b_ids.p; int32_t* d_mi = d_pi + n; int32_t* d_pt = d_mi + n;
  const int pc = (int)std::min<int64_t>(npix, c.opt.batch_paths);
  hipError_t e;
  if (npix > 0 && ensure_paths(path_floats((size_t)pc, 1, false) * 4 + 256, /*may_spread=*/false, &e)) return fail(std::string("hipMalloc(&b.p, bytes): ") + hipGetErrorString(e));
  for (int px0 = 0; px0 < npix; px0 += pc) {
    const int pn = std::min(pc, npix - px0);
    DevPaths bank[2]; std::memset(bank, 0, sizeof bank);
    carve(bank, pn, 1, false);
    DevPaths q = bank[0];
    q.P = pn; q.npix = pn; q.pixmap = (const uint32_t*)c.b_pixmap.p + px0; q.sample_base = 0; q.slot_id = nullptr; q.final_flags = q.flags;
    launch_raygen(c.stream, F, c.scene, q);
    if (trace(q, pn, pass_launch())) return 1;
    launch_debug(c.stream, F, c.scene, q, accum_ptr(), d_pi, d_mi, d_pt);
  }
  HIP_TRY(hipGetLastError());
  // ray_tracer.adb:249-257: the debug image is resolved without dividing by spp
  if (download_from(accum_ptr(), accum_host, screen_host, p->layout, 1)) return 1;
  auto copy_ids = [&](int32_t* host, const int32_t* dev) -> int {
    if (!host) return 0;
    if (p->layout == ART_LAYOUT_ADA_XY) {
      if (ensure(c.b_stage, n * 12)) return 1;
      launch_to_xmajor_u32(c.stream, (const uint32_t*)dev, (uint32_t*)c.b_stage.p, c.width, c.height);
      HIP_TRY(hipMemcpyAsync(host, c.b_stage.p, n * 4, hipMemcpyDeviceToHost, c.stream));
    } else HIP_TRY(hipMemcpyAsync(host, dev, n * 4, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return 0;
  };
  if (copy_ids(prim_index, d_pi) || copy_ids(mat_id, d_mi) || copy_ids(prim_type, d_pt)) return 1;
  return synchronize_one();
}

// Debug_Ray_Tracing is one primary ray per pixel: in multi-device mode device 0 takes the whole frame for it (its tile ownership is
// restored afterwards) -- there is nothing to shard.
int debug_pass(const ArtPassParams* p, float* accum_host, uint32_t* screen_host, int32_t* prim_index, int32_t* mat_id, int32_t* prim_type) {
  if (g_ndev == 1) return debug_pass_one(p, accum_host, screen_host, prim_index, mat_id, prim_type);
  Dev0Guard guard;
  if (use_dev(0)) return 1;
  Ctx& c = g_ctx;
  const int rank = c.rank, nranks = c.nranks;
  c.rank = 0; c.nranks = 1;
  int rc = (c.width > 0) ? build_shard() : 0;
  if (!rc) rc = debug_pass_one(p, accum_host, screen_host, prim_index, mat_id, prim_type);
  c.rank = rank; c.nranks = nranks;
  if (c.width > 0 && build_shard()) return 1;
  return rc;
}

}  // namespace art
