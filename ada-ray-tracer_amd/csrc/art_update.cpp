// art_update.cpp -- the device-side scene updates of the C ABI (include/art_hip.h): art_refit_device (art_refit.hip), art_rebuild_device
// (art_rebuild.hip + the GPU builders), art_move_instances_device, art_refit_mesh_device, art_rebuild_instance_tree_device and
// art_rebuild_mesh_tree_device (art_move.hip), art_get_tree_cost, art_get_instance_tree_cost, art_get_mesh_tree_cost and the diagnostic art_export_two_level.  What the kinds share is written
// once, in the first half of this file: the ordering of the caller's stream against the context stream (StreamOrder), the per-context
// lane of timing event pairs (art_event_pairs.h) and bad-item bookkeeping (UpdateLane), and the driver that runs an update on every context (run_update).
// The three calls that replace a tree have a driver of their own (run_rebuild), which states the rule that makes them safe.
// Invariants of every entry point: every check comes before the first launch; the end event of a timed update is recorded on every way
// out; the context stream is ordered after the update also when a launch failed; device 0 is current on every exit path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "art_api_internal.h"
#include "art_rebuild.h"
#include "art_refit.h"
#include "art_lbvh.h"
#include "art_renumber.h"

namespace art {

static ArtRefitInfo g_refit_info = ArtRefitInfo();         // art_get_refit_info: cumulative since the last upload
static ArtRebuildInfo g_rebuild_info = ArtRebuildInfo();   // art_get_rebuild_info: the same
static ArtMoveInfo g_move_info = ArtMoveInfo();            // art_get_move_info: the same
static ArtMeshRefitInfo g_mesh_refit_info = ArtMeshRefitInfo();   // art_get_mesh_refit_info: the same
static ArtInstanceRebuildInfo g_inst_rebuild_info = ArtInstanceRebuildInfo();   // art_get_instance_rebuild_info: the same
static ArtMeshRebuildInfo g_mesh_rebuild_info = ArtMeshRebuildInfo();           // art_get_mesh_rebuild_info: the same
void reset_update_info() { g_refit_info = ArtRefitInfo(); g_rebuild_info = ArtRebuildInfo(); g_move_info = ArtMoveInfo(); g_mesh_refit_info = ArtMeshRefitInfo(); g_inst_rebuild_info = ArtInstanceRebuildInfo(); g_mesh_rebuild_info = ArtMeshRebuildInfo(); }
// ---- the caller's stream ----------------------------------------------------------------------------------------------------------
StreamOrder::StreamOrder(Ctx& ctx, hipStream_t st) : c(ctx), cs(ctx.stream), qs(st == nullptr ? ctx.stream : (st == hipStreamLegacy ? nullptr : st)) {}
int StreamOrder::enter() {
  if (!other()) return 0;
  for (hipEvent_t& e : c.q_ev) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c.q_ev[0], cs));
  HIP_TRY(hipStreamWaitEvent(qs, c.q_ev[0], 0));
  return 0;
}
int StreamOrder::leave() {              // what was enqueued stays ordered before the context stream's next work
  if (!other()) return 0;
  HIP_TRY(hipEventRecord(c.q_ev[1], qs));
  HIP_TRY(hipStreamWaitEvent(cs, c.q_ev[1], 0));
  return 0;
}

// ---- the lane of one kind of update in one context --------------------------------------------------------------------------------
// the current context's part of a new plan: contexts k > 0 stage the caller's data, device 0 signals when that data is ready
static int plan_lane(UpdateLane& L, size_t stage_bytes) {
  if (g_cur != &g_devs[0]) {
    if (ensure(L.b_stage, stage_bytes)) return 1;
    if (!L.done_ev) HIP_TRY(hipEventCreateWithFlags(&L.done_ev, hipEventDisableTiming));
  } else if (g_ndev > 1 && !L.ready_ev) HIP_TRY(hipEventCreateWithFlags(&L.ready_ev, hipEventDisableTiming));
  return 0;
}

// Completed event pairs -> ms_sum (device 0's; the other contexts' times are not reported).  wait: every pair is waited for; else pairs
// still in flight stay listed, so that a host that updates every frame and never synchronises keeps a list as long as the updates in flight.
static int fold_lane(UpdateLane& L, bool wait, double& ms_sum) {
  const bool dev0 = (g_cur == &g_devs[0]);
  const hipError_t e = L.pairs.fold(wait, [&ms_sum, dev0](float ms, uint8_t) { if (dev0) ms_sum += ms; });
  return e == hipSuccess ? 0 : fail(std::string("update event pair: ") + hipGetErrorString(e));
}

// A timed update on stream s: the lane's completed pairs are folded, a new one ends when `timer` leaves scope; the lane is unread.
static int start_lane(UpdateLane& L, hipStream_t s, double& ms_sum, EventPairs::Timer& timer) {
  (void)fold_lane(L, /*wait=*/false, ms_sum);
  HIP_TRY(L.pairs.begin(timer, s));
  L.unread = true;
  return 0;
}

static void release_lane(UpdateLane& L) {
  L.b_stage.release();
  L.pairs.release();
  L.unread = false; L.bad_last = 0; L.bad_reported = true;
}
static void destroy_lane(UpdateLane& L) {
  release_lane(L);
  L.pairs.destroy();
  for (hipEvent_t e : {L.ready_ev, L.done_ev}) if (e) (void)hipEventDestroy(e);
  L.ready_ev = L.done_ev = nullptr;
}

// reported once per bad update, like a lost path; the boxes stay empty until a good update or an upload
static int report_bad(UpdateLane& L, const char* head, const char* tail) {
  if (L.bad_reported) return 0;
  L.bad_reported = true;
  return fail(head + std::to_string(L.bad_last) + tail);
}

// ---- one update on every context --------------------------------------------------------------------------------------------------
// The driver of refit and move, after the kind's own refusals.  Every check comes before the first launch: the caller's buffers (planes),
// then every context's plan (plan(), with that context current).  Device 0 runs `work` on the caller's stream, ordered against its context
// stream; every other context waits for the caller's stream, copies the sources from device 0 into its lane's stage (one after the other; a
// null source keeps its place), runs `work` on its own stream, and the caller's stream waits for it -- so the caller may overwrite its
// buffers after whatever it enqueues next.  mark() notes on the host that the scene changes.
template <typename Lane, typename Plan, typename Mark, typename Work>
static int run_update(const std::string& call, hipStream_t st, Lane lane, std::initializer_list<DevPlane> planes, Plan plan, Mark mark, Work work) {
  Ctx& c0 = g_devs[0];
  Dev0Guard guard;
  if (use_dev(0)) return 1;
  if (check_planes(planes)) return 1;
  const DevPlane* const srcs = planes.begin();
  std::vector<const void*> at;
  for (const DevPlane& x : planes) at.push_back(x.p);
  for (int k = 0; k < g_ndev; ++k) { if (use_dev(k) || plan()) return 1; }
  if (use_dev(0)) return 1;
  StreamOrder order(c0, st);
  if (order.enter()) return 1;
  mark();
  const hipStream_t qs = order.qs;
  int rc = 0;
  if (g_ndev > 1 && hipEventRecord(lane(c0).ready_ev, qs) != hipSuccess) rc = fail(call + ": hipEventRecord failed");
  if (!rc) rc = work(at.data(), qs);
  for (int k = 1; k < g_ndev && !rc; ++k) {
    if (use_dev(k)) { rc = 1; break; }
    Ctx& c = g_ctx;
    UpdateLane& L = lane(c);
    bool ok = hipStreamWaitEvent(c.stream, lane(c0).ready_ev, 0) == hipSuccess;
    char* stage = (char*)L.b_stage.p;
    for (size_t i = 0; i < planes.size(); stage += srcs[i].bytes, ++i) {
      at[i] = srcs[i].p ? stage : nullptr;
      if (ok && srcs[i].p) ok = hipMemcpyPeerAsync(stage, c.device, srcs[i].p, c0.device, srcs[i].bytes, c.stream) == hipSuccess;
    }
    if (!ok) { rc = fail(call + ": copy to device " + std::to_string(c.device) + " failed"); break; }
    rc = work(at.data(), c.stream);
    if (hipEventRecord(L.done_ev, c.stream) != hipSuccess || hipStreamWaitEvent(qs, L.done_ev, 0) != hipSuccess) rc = rc ? rc : fail(call + ": event ordering failed");
  }
  if (use_dev(0) || order.leave()) return 1;          // (also after a failure)
  return rc;
}

// the info getters: cumulative since the upload; they wait for every context's stream (an update on another stream is ordered before it)
template <typename Info, typename Fold>
static int get_info(Info* out, const char* null_msg, const Info& info, Fold fold) {
  if (!out) return fail(null_msg);
  Dev0Guard guard;
  for (int k = 0; k < g_ndev; ++k) {
    if (use_dev(k)) return 1;
    if (!g_ctx.device_ready) continue;
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    if (fold()) return 1;
  }
  *out = info;
  return 0;
}

// ---- what refit and rebuild share -------------------------------------------------------------------------------------------------
struct MeshCall { const char *name, *noun, *done; };
static const MeshCall kRefitCall = {"art_refit_device", "refit", "refitted"}, kRebuildCall = {"art_rebuild_device", "rebuild", "rebuilt"};
// the refusals both open with
static int check_mesh_update(const MeshCall& call, const float* pos, int64_t nverts) {
  const Ctx& c0 = g_devs[0]; const std::string name = call.name;
  if (!c0.scene_ready) return fail(name + ": no scene uploaded");
  const HostScene& hs = c0.host_scene;
  if (c0.scene.n_inst > 0) return fail(name + ": the scene is instanced (n_instances > 0); only the tree of a flat CLOSEST mesh is " + call.done);
  if (hs.m_nverts == 0) return fail(name + ": the scene has no ART_MESH_CLOSEST mesh");
  if (hs.gcore_seam) return fail(name + ": the scene was committed through gcore_commit_scene, whose host copy of the tree a " + call.noun + " would leave stale");
  if (nverts != hs.m_nverts) return fail(name + ": nverts " + std::to_string(nverts) + " differs from the uploaded mesh's " + std::to_string(hs.m_nverts));
  if (!pos) return fail(name + ": null pos3f");
  return 0;
}

// the tree in HBM changes: the host copies of it (art_export_bvh's cache, a host-built tree) and of the positions are stale
static void drop_stale_host_copies(HostScene& hs) {
  std::vector<float>().swap(hs.bvh.nodes); std::vector<float>().swap(hs.bvh.tris); std::vector<uint32_t>().swap(hs.bvh.qnodes);
  std::vector<float>().swap(hs.m_pos);
}

// ---- moving geometry (art_refit_device, art_refit.hip) ----------------------------------------------------------------------------
// The plan of the current context: its tree's inner nodes grouped by depth (read back from HBM once: the GPU builders leave the tree
// there only, and every builder orders its nodes differently), the mesh's index triples, the tight-box scratch and the counters.
static int build_refit_plan(const HostScene& hs) {
  Ctx& c = g_ctx;
  Ctx::RefitPlan& R = c.refit;
  const auto t0 = std::chrono::steady_clock::now();
  const int W = c.scene.node_width, NF = node_floats(W), N = c.scene.n_nodes;
  if (N < 1 || !c.b_nodes.p) return fail("art_refit_device: the scene has no tree");
  std::vector<float> nodes((size_t)N * NF);
  HIP_TRY(hipStreamSynchronize(c.stream));
  HIP_TRY(hipMemcpy(nodes.data(), c.b_nodes.p, nodes.size() * 4, hipMemcpyDeviceToHost));
  std::vector<int32_t> order;                                   // breadth first: level L = order[level_off[L] .. level_off[L + 1])
  R.level_off.clear();
  static const char* const wrong[] = {nullptr, "a leaf outside the triangle records", "the uploaded nodes do not form a tree", "unreachable nodes in the uploaded tree"};
  const TreeFault fault = walk_levels(nodes.data(), W, 0, N, c.scene.n_tris, kMaxLeafTris, order, R.level_off, [](int32_t) {});
  if (fault != TreeFault::none) return fail(std::string("art_refit_device: internal: ") + wrong[(int)fault]);
  if (upload(R.b_idx, hs.m_idx) || upload(R.b_levels, order) || ensure(R.b_tight, (size_t)N * 6 * sizeof(float)) || ensure(R.b_bad, 2 * sizeof(unsigned long long)))
    return 1;
  HIP_TRY(hipMemset(R.b_bad.p, 0, 2 * sizeof(unsigned long long)));
  if (plan_lane(R.lane, 2 * 12 * (size_t)hs.m_nverts)) return 1;
  g_refit_info.plan_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  R.ready = true;
  return 0;
}

// art_render_aovs_motion_device reads the plan's index triples: the current context's plan, built here when no refit has built it since the
// upload or the last rebuild (the host then waits for the context stream, as the first refit does)
int ensure_refit_plan() { return !g_ctx.refit.ready && build_refit_plan(g_devs[0].host_scene); }

// the current context's refit on stream s, from positions (and normals) in this context's device memory
static int refit_one(const HostScene& hs, const float* pos, const float* nrm, hipStream_t s) {
  Ctx& c = g_ctx;
  Ctx::RefitPlan& P = c.refit;
  RefitArgs A;
  std::memset(&A, 0, sizeof A);
  A.pos3f = pos; A.nrm3f = nrm; A.idx = (const int32_t*)P.b_idx.p;
  A.nverts = hs.m_nverts; A.n_prims = (int32_t)(hs.m_idx.size() / 3); A.n_recs = c.scene.n_tris;
  A.tris = (float*)c.b_tris.p; A.qtris = (float*)c.b_qtris.p; A.m_shade = (float*)c.b_m_shade.p;
  A.bad = (unsigned long long*)P.b_bad.p;
  A.nodes = (float*)c.b_nodes.p; A.qnodes = (c.scene.node_width == 4) ? (QNode*)c.b_qnodes.p : nullptr;
  A.tight = (float*)P.b_tight.p;
  A.width = c.scene.node_width; A.inflate_rel = c.opt.bvh_params.inflate_rel; A.inflate_abs = c.opt.bvh_params.inflate_abs;
  EventPairs::Timer timer;
  if (start_lane(P.lane, s, g_refit_info.refit_ms, timer)) return 1;
  HIP_TRY(hipMemsetAsync(A.bad, 0, sizeof(unsigned long long), s));      // [0]: this refit's bad vertices ([1] counts since the upload)
  launch_refit_tris(s, A);
  for (int L = (int)P.level_off.size() - 2; L >= 0; --L)                 // deepest level first
    launch_refit_level(s, A, (const int32_t*)P.b_levels.p + P.level_off[(size_t)L], P.level_off[(size_t)L + 1] - P.level_off[(size_t)L]);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(std::string("art_refit_device: kernel launch failed: ") + hipGetErrorString(e));
  return 0;
}

// The current context's event pairs of one kind (all of them: its stream is idle, and an update on another stream is ordered before the
// context stream's later work), then the kind's counters where an update has not been read yet: read(words) -> this update's bad items.
template <int N, typename Read>
static int fold_kind(UpdateLane& L, double& ms_sum, const void* counters, Read read) {
  const bool dev0 = (g_cur == &g_devs[0]);
  if (fold_lane(L, /*wait=*/true, ms_sum)) return 1;
  if (!L.unread || !counters) return 0;
  unsigned long long w[N];
  HIP_TRY(hipMemcpy(w, counters, sizeof w, hipMemcpyDeviceToHost));
  L.unread = false;
  L.bad_last = read(w, dev0); L.bad_reported = (L.bad_last == 0);
  return 0;
}
static int fold_refit() {                   // b_bad: [0] this refit's bad vertices, [1] since the upload
  Ctx::RefitPlan& R = g_ctx.refit;
  return fold_kind<2>(R.lane, g_refit_info.refit_ms, R.b_bad.p, [&](const unsigned long long* w, bool dev0) { R.bad_total = w[1]; if (dev0) g_refit_info.bad_vertices = w[1]; return w[0]; });
}

int refit_device(const float* pos, const float* nrm, int64_t nverts, hipStream_t st) {
  if (check_mesh_update(kRefitCall, pos, nverts)) return 1;
  HostScene& hs = g_devs[0].host_scene;
  const size_t bytes = 12 * (size_t)nverts;
  return run_update(kRefitCall.name, st, [](Ctx& c) -> UpdateLane& { return c.refit.lane; }, {{pos, bytes, "pos3f"}, {nrm, bytes, "nrm3f"}},
                    [&] { return !g_ctx.refit.ready && build_refit_plan(hs); },
                    [&] { drop_stale_host_copies(hs); hs.refitted = true; if (nrm) hs.m_shade_stale = true; g_refit_info.refits += 1; },   // (art_trace_rays reads the shading records on the host)
                    [&](const void* const* src, hipStream_t s) { return refit_one(hs, (const float*)src[0], (const float*)src[1], s); });
}

int get_refit_info(ArtRefitInfo* out) { return get_info(out, "null ArtRefitInfo", g_refit_info, fold_refit); }

// ---- an instanced scene changes (art_move_instances_device, art_refit_mesh_device, art_move.hip) ----------------------------------
// The parts of a plan that are built on the host, as one buffer: every section is 16-byte aligned, a null source reserves zeroed scratch.
struct PlanImage {
  std::vector<uint8_t> img;
  size_t put(const void* p, size_t bytes) { const size_t at = img.size(); img.resize(at + ((bytes + 15) & ~(size_t)15), 0); if (p && bytes) std::memcpy(&img[at], p, bytes); return at; }
  int upload_to(DevBuf& b) const { return upload(b, img); }
};

// a context's arrays in HBM have the sizes of the two-level build the host keeps (build_move_plan, export_two_level)
static bool arrays_are_the_kept_builds(const Ctx& c, const TwoLevelHost& T) {
  const size_t n_entry = T.entry.size(), n_tlas = (size_t)T.tlas.n_nodes, n_blas = T.blas_nodes.size() / 32;
  return c.b_inst.bytes == n_entry * sizeof(DevInstance) && c.b_qnodes.bytes == (n_tlas + n_blas) * kQNodeBytes && c.b_tlas_nodes.bytes == n_tlas * 128 &&
         c.b_blas_nodes.bytes == n_blas * 128 && c.b_tlas_tris.bytes == n_entry * kTriBytes && c.b_blas_tris.bytes == T.blas_tris.size() * 4;
}

// The plan of the current context, from the two-level build the upload kept and before either call has changed anything: MovePlanHost's
// constant arrays and the meshes' index triples in one buffer, what the kernels maintain in another (the tight boxes, the meshes' boxes
// and pads, the matrices in force), and MoveArgs pointing into both and into the scene's arrays.  `call` builds it; its info takes the time.
static int build_move_plan(const HostScene& hs, const std::string& call, double& plan_ms) {
  Ctx& c = g_ctx;
  Ctx::MovePlan& P = c.move;
  const auto t0 = std::chrono::steady_clock::now();
  MovePlanHost H;
  std::string err;
  if (!build_move_plan_host(hs.two, H, err)) return fail(call + ": " + err);
  const size_t n_entry = hs.two.entry.size(), n_inst = hs.two.inst.size(), nm = (size_t)H.n_mesh, n_tlas = (size_t)hs.two.tlas.n_nodes, n_blas = H.node_mesh.size();
  if (!arrays_are_the_kept_builds(c, hs.two)) return fail(call + ": internal: the arrays in HBM are not the kept build's");
  if (hs.inst.size() != n_entry || hs.mesh_nverts.size() != nm || hs.mesh_idx_off.size() != nm + 1 || c.b_qtris.bytes != hs.two.blas_tris.size() / kTriFloats * (size_t)kQTriBytes)
    return fail(call + ": internal: the host scene is not the kept build's");
  PlanImage img, work;                                                     // the constant arrays | what the kernels maintain
  const size_t o_roff = img.put(H.range_off.data(), H.range_off.size() * 4), o_rng = img.put(H.ranges.data(), H.ranges.size() * 4), o_prox = img.put(H.proxy_rec.data(), H.proxy_rec.size() * 4);
  const size_t o_imesh = img.put(H.inst_mesh.data(), H.inst_mesh.size() * 4), o_mbase = img.put(H.mesh_base.data(), H.mesh_base.size() * 4);
  const size_t o_nmesh = img.put(H.node_mesh.data(), H.node_mesh.size() * 4), o_lev = img.put(H.tlas_levels.data(), H.tlas_levels.size() * 4);
  const size_t o_blev = img.put(H.blas_levels.data(), H.blas_levels.size() * 4), o_idx = img.put(hs.mesh_idx.data(), hs.mesh_idx.size() * 4);
  if (img.upload_to(P.b_plan)) return 1;
  auto room = [&](size_t bytes) { return work.put(nullptr, bytes); };
  const size_t w_state = room(kMoveStateWords * 8), w_need = room(nm * 8), w_mbad = room(nm * 8), w_tight = room(n_tlas * 24), w_box = room(n_entry * 24), w_ok = room(n_inst * 4), w_pad = work.put(H.pad_abs.data(), nm * 4), w_repad = room(nm * 4);
  const size_t w_mbox = work.put(H.mesh_box.data(), nm * 24), w_btight = work.put(H.blas_tight.data(), n_blas * 24), w_mcur = room(n_inst * 48);
  for (size_t i = 0; i < n_inst; ++i) std::memcpy(&work.img[w_mcur + 48 * i], hs.inst[i].m, 48);      // (record i < n_inst is instance i; no move has been accepted yet)
  if (work.upload_to(P.b_work)) return 1;
  const char* pb = (const char*)P.b_plan.p; char* wb = (char*)P.b_work.p;
  MoveArgs& A = P.args;
  A = MoveArgs();
  A.n_inst = (int32_t)n_inst; A.n_entry = (int32_t)n_entry; A.n_mesh = (int32_t)nm; A.n_blas_nodes = (int32_t)n_blas;
  A.inst = (DevInstance*)c.b_inst.p; A.tlas_nodes = (float*)c.b_tlas_nodes.p; A.tlas_tris = (float*)c.b_tlas_tris.p;
  A.blas_nodes = (float*)c.b_blas_nodes.p; A.blas_tris = (const float*)c.b_blas_tris.p; A.qnodes = (QNode*)c.b_qnodes.p;
  A.range_off = (const int32_t*)(pb + o_roff); A.ranges = (const int32_t*)(pb + o_rng); A.proxy_rec = (const int32_t*)(pb + o_prox); A.inst_mesh = (const int32_t*)(pb + o_imesh);
  A.mesh_base = (const int32_t*)(pb + o_mbase); A.node_mesh = (const int32_t*)(pb + o_nmesh);
  A.mesh_box = (float*)(wb + w_mbox); A.blas_tight = (float*)(wb + w_btight); A.m_cur = (float*)(wb + w_mcur);
  A.state = (unsigned long long*)(wb + w_state); A.needed = (unsigned long long*)(wb + w_need); A.mesh_bad = (unsigned long long*)(wb + w_mbad); A.tlas_tight = (float*)(wb + w_tight); A.ent_box = (float*)(wb + w_box);
  A.inst_ok = (int32_t*)(wb + w_ok); A.pad_cur = (float*)(wb + w_pad); A.repad = (int32_t*)(wb + w_repad);
  A.extent = (double)hs.two.scene_extent; A.mesh_pad_rel = hs.two.mesh_pad_rel; A.mesh_pad_min = hs.two.mesh_pad_min;
  const BvhBuildParams tp;                                                 // the instance tree builder's pad rule: the defaults, as build_two_level_host applied them
  A.tlas_pad_rel = tp.inflate_rel; A.tlas_pad_abs = tp.inflate_abs;
  P.levels = (const int32_t*)(pb + o_lev); P.level_off = H.tlas_level_off; P.n_tlas = (int32_t)n_tlas;
  P.small_entries = H.records <= 64 * (int64_t)n_entry;
  P.blas_levels = (const int32_t*)(pb + o_blev); P.blas_level_off = H.blas_level_off;
  P.meshes.assign(nm, Ctx::MovePlan::Mesh());
  int64_t max_verts = 0;
  for (size_t mi = 0; mi < nm; ++mi) {
    Ctx::MovePlan::Mesh& m = P.meshes[mi];
    m.nverts = hs.mesh_nverts[mi]; m.level_first = H.mesh_level_first[mi]; m.level_end = H.mesh_level_first[mi + 1];
    m.n_prims = (int32_t)((hs.mesh_idx_off[mi + 1] - hs.mesh_idx_off[mi]) / 3);
    m.idx = (const int32_t*)(pb + o_idx) + hs.mesh_idx_off[mi];
    max_verts = std::max(max_verts, m.nverts);
  }
  for (size_t i = 0; i < n_inst; ++i) {                                    // (build_move_plan_host checked every instance's slice)
    Ctx::MovePlan::Mesh& m = P.meshes[(size_t)hs.two.inst[i].mesh];
    m.tri_base = hs.two.inst[i].tri_base; m.n_recs = hs.two.inst[i].n_tris; m.shade_base = hs.inst[i].shade_base;
    if (m.n_prims < 1 || (size_t)(m.shade_base + m.n_prims) * kTriShadeFloats * 4 > c.b_m_shade.bytes) return fail(call + ": internal: a mesh's shading records lie outside the array");
  }
  if (plan_lane(P.lane, 48 * n_inst) || plan_lane(P.refit_lane, 2 * 12 * (size_t)max_verts)) return 1;
  plan_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  P.ready = true;
  return 0;
}

// matrices, pads, re-pad, entry-point boxes, the instance tree: what a move and a mesh refit both end in
static void launch_move_pipeline(const Ctx::MovePlan& P, const MoveArgs& A, hipStream_t s) {
  launch_move_matrices(s, A);
  launch_move_repad(s, A);
  launch_move_entry_boxes(s, A, P.small_entries);
  for (int L = (int)P.level_off.size() - 2; L >= 0; --L)                   // deepest level first
    launch_move_tlas_level(s, A, P.levels + P.level_off[(size_t)L], P.level_off[(size_t)L + 1] - P.level_off[(size_t)L]);
}

// the current context's move on stream s, from matrices in this context's device memory
static int move_one(const float* m12f, hipStream_t s) {
  Ctx& c = g_ctx;
  Ctx::MovePlan& P = c.move;
  MoveArgs A = P.args;
  A.m12f = m12f; A.m_cur_out = A.m_cur; A.bad_total = A.state + 2; A.repads = A.state + 3;
  EventPairs::Timer timer;
  if (start_lane(P.lane, s, g_move_info.move_ms, timer)) return 1;
  launch_move_pipeline(P, A, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(std::string("art_move_instances_device: kernel launch failed: ") + hipGetErrorString(e));
  return 0;
}

static int fold_move() {                    // the counters k_move_matrices / k_move_pads_mesh keep
  Ctx::MovePlan& P = g_ctx.move;
  return fold_kind<4>(P.lane, g_move_info.move_ms, P.args.state, [&](const unsigned long long* w, bool dev0) { if (dev0) { g_move_info.bad_matrices = w[2]; g_move_info.repads = w[3]; } return w[1]; });
}

int move_instances_device(const float* m12f, int64_t n_instances, hipStream_t st) {
  Ctx& c0 = g_devs[0];
  if (!c0.scene_ready) return fail("art_move_instances_device: no scene uploaded");
  HostScene& hs = c0.host_scene;
  if (hs.gcore_seam) return fail("art_move_instances_device: the scene was committed through gcore_commit_scene, which keeps its own instances");
  if (c0.scene.n_inst <= 0) return fail("art_move_instances_device: the scene is not instanced (n_instances = 0); art_refit_device moves the vertices of a flat mesh");
  if (n_instances != (int64_t)c0.scene.n_inst) return fail("art_move_instances_device: n_instances " + std::to_string(n_instances) + " differs from the uploaded scene's " + std::to_string(c0.scene.n_inst));
  if (!m12f) return fail("art_move_instances_device: null m12f");
  return run_update("art_move_instances_device", st, [](Ctx& c) -> UpdateLane& { return c.move.lane; }, {{m12f, 48 * (size_t)n_instances, "m12f"}},
                    [&] { return !g_ctx.move.ready && build_move_plan(hs, "art_move_instances_device", g_move_info.plan_ms); },
                    [&] { hs.inst_stale = true; g_move_info.moves += 1; },                                      // (art_trace_rays reads the matrices on the host)
                    [&](const void* const* src, hipStream_t s) { return move_one((const float*)src[0], s); });
}

// ---- the camera of the uploaded scene (art_set_camera) ------------------------------------------------------------------------------
// What depends on the camera: cam_pos / cam_matrix of the scene header -- the host's copy (Ctx::scene), which raygen, shade, the AOV and
// the query kernels take by value at launch, and the copy in HBM (d_scene) the trace kernels take by pointer (they do not read the
// camera; it is kept equal) -- and, on an instanced scene, the scene extent (art_host_scene.cpp: the largest |coordinate| a ray can start
// at), which the absolute pad of every mesh's boxes follows (art_move.hip k_move_pads_inst).  Pads only grow, as for a move: a camera
// inside the extent the pads were made for changes nothing else; one outside it raises the extent and runs the move pipeline at the
// matrices in force (pads, re-pad of the meshes that outgrow theirs, entry-point boxes, instance tree).  The flat tree, the BF mesh, the
// spheres, lights and materials, the pixel map and the path state do not depend on the camera.
static void set_camera_one(Ctx& c, const CameraWords& w, hipStream_t s) {
  std::memcpy(c.scene.cam_pos, w.w, 12); std::memcpy(c.scene.cam_matrix, w.w + 3, 64);
  launch_set_camera(s, c.d_scene, w);
}

int set_camera(const float* cam_pos, const float* cam_matrix) {
  const std::string name = "art_set_camera";
  Ctx& c0 = g_devs[0];
  if (!c0.scene_ready) return fail(name + ": no scene uploaded");
  HostScene& hs = c0.host_scene;
  if (hs.gcore_seam) return fail(name + ": the scene was committed through gcore_commit_scene, which has no camera");
  if (!cam_pos || !cam_matrix) return fail(name + ": null cam_pos or cam_matrix");
  CameraWords w;
  std::memcpy(w.w, cam_pos, 12); std::memcpy(w.w + 3, cam_matrix, 64);
  for (float v : w.w) if (!std::isfinite(v)) return fail(name + ": a component of the camera is not finite");
  float extent = hs.extent_rest;
  for (int k = 0; k < 3; ++k) extent = std::max(extent, std::fabs(cam_pos[k]));
  const bool grow = c0.scene.n_inst > 0 && extent > hs.two.scene_extent;
  auto note = [&] { std::memcpy(hs.hdr.cam_pos, w.w, 12); std::memcpy(hs.hdr.cam_matrix, w.w + 3, 64); };
  if (!grow) {                             // every context's header, on its own stream: no plan, no wait
    Dev0Guard guard;
    for (int k = 0; k < g_ndev; ++k) {
      if (use_dev(k)) return 1;
      set_camera_one(g_ctx, w, g_ctx.stream);
      if (hipGetLastError() != hipSuccess) return fail(name + ": kernel launch failed");
    }
    note();
    return 0;
  }
  // the camera leaves the extent the pads were made for (the first update after an upload builds the plan a move shares, and waits for it)
  return run_update(name, nullptr, [](Ctx& c) -> UpdateLane& { return c.move.lane; }, {},
                    [&] { return !g_ctx.move.ready && build_move_plan(hs, name, g_move_info.plan_ms); },
                    [&] { note(); hs.two.scene_extent = extent; },
                    [&](const void* const*, hipStream_t s) {
                      Ctx& c = g_ctx;
                      set_camera_one(c, w, s);
                      c.move.args.extent = (double)extent;
                      MoveArgs A = c.move.args;
                      A.m12f = A.m_cur; A.m_cur_out = nullptr; A.bad_total = nullptr; A.repads = A.state + 3;      // (a re-pad counts with the moves')
                      launch_move_pipeline(c.move, A, s);
                      return hipGetLastError() == hipSuccess ? 0 : fail(name + ": kernel launch failed");
                    });
}

int get_move_info(ArtMoveInfo* out) { return get_info(out, "null ArtMoveInfo", g_move_info, fold_move); }

// ---- deforming a mesh of an instanced scene (art_refit_mesh_device, art_refit.hip + art_move.hip) ---------------------------------
// the current context's mesh refit on stream s, from positions (and normals) in this context's device memory
static int refit_mesh_one(int32_t mesh, const float* pos, const float* nrm, hipStream_t s) {
  Ctx& c = g_ctx;
  Ctx::MovePlan& P = c.move;
  const Ctx::MovePlan::Mesh& m = P.meshes[(size_t)mesh];
  MoveArgs A = P.args;
  A.m12f = A.m_cur; A.m_cur_out = nullptr; A.bad_total = nullptr; A.repads = A.state + 6;
  RefitArgs R;                                                             // k_refit_tris on the mesh's slices of the records, their padded copy and the shading records
  std::memset(&R, 0, sizeof R);
  R.pos3f = pos; R.nrm3f = nrm; R.idx = m.idx;
  R.nverts = m.nverts; R.n_prims = m.n_prims; R.n_recs = m.n_recs;
  R.tris = (float*)c.b_blas_tris.p + (size_t)kTriFloats * (size_t)m.tri_base; R.qtris = (float*)c.b_qtris.p + (size_t)(kQTriBytes / 4) * (size_t)m.tri_base;
  R.m_shade = (float*)c.b_m_shade.p + (size_t)kTriShadeFloats * (size_t)m.shade_base;
  R.bad = A.state + 4;                                                     // state[4]: this refit's bad vertices, state[5]: since the upload
  EventPairs::Timer timer;
  if (start_lane(P.refit_lane, s, g_mesh_refit_info.refit_ms, timer)) return 1;
  HIP_TRY(hipMemsetAsync(R.bad, 0, sizeof(unsigned long long), s));
  launch_refit_tris(s, R);
  for (int L = m.level_end - 1; L >= m.level_first; --L)                   // the mesh's tree, deepest level first
    launch_refit_mesh_level(s, A, P.blas_levels + P.blas_level_off[(size_t)L], P.blas_level_off[(size_t)L + 1] - P.blas_level_off[(size_t)L]);
  launch_refit_mesh_box(s, A, mesh);
  launch_move_pipeline(P, A, s);                                           // at the matrices in force
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(std::string("art_refit_mesh_device: kernel launch failed: ") + hipGetErrorString(e));
  return 0;
}

static int fold_mesh_refit() {              // the counters k_refit_tris / k_refit_mesh_box / k_move_pads_mesh keep for the mesh refits; reported: the bad vertices the meshes hold now
  Ctx::MovePlan& P = g_ctx.move;
  return fold_kind<kMoveStateWords>(P.refit_lane, g_mesh_refit_info.refit_ms, P.args.state, [&](const unsigned long long* w, bool dev0) { if (dev0) { g_mesh_refit_info.bad_vertices = w[5]; g_mesh_refit_info.repads = w[6]; } return w[7]; });
}

int refit_mesh_device(int32_t mesh, const float* pos, const float* nrm, int64_t nverts, hipStream_t st) {
  Ctx& c0 = g_devs[0];
  const std::string name = "art_refit_mesh_device";
  if (!c0.scene_ready) return fail(name + ": no scene uploaded");
  HostScene& hs = c0.host_scene;
  if (hs.gcore_seam) return fail(name + ": the scene was committed through gcore_commit_scene, which keeps its own meshes");
  if (c0.scene.n_inst <= 0) return fail(name + ": the scene is not instanced (n_instances = 0); art_refit_device moves the vertices of a flat mesh");
  const int64_t n_mesh = (int64_t)hs.mesh_nverts.size();
  if (mesh < 0 || mesh >= n_mesh) return fail(name + ": mesh " + std::to_string(mesh) + " is out of range (the scene has " + std::to_string(n_mesh) + " meshes)");
  if (hs.mesh_idx_off[(size_t)mesh + 1] == hs.mesh_idx_off[(size_t)mesh]) return fail(name + ": no instance shows mesh " + std::to_string(mesh));
  if (nverts != (int64_t)hs.mesh_nverts[(size_t)mesh]) return fail(name + ": nverts " + std::to_string(nverts) + " differs from the uploaded mesh's " + std::to_string(hs.mesh_nverts[(size_t)mesh]));
  if (!pos) return fail(name + ": null pos3f");
  const size_t bytes = 12 * (size_t)nverts;
  return run_update(name, st, [](Ctx& c) -> UpdateLane& { return c.move.refit_lane; }, {{pos, bytes, "pos3f"}, {nrm, bytes, "nrm3f"}},
                    [&] { return !g_ctx.move.ready && build_move_plan(hs, name, g_mesh_refit_info.plan_ms); },
                    [&] { if (nrm) hs.m_shade_stale = true; g_mesh_refit_info.refits += 1; },                     // (art_trace_rays reads the shading records on the host; the instance table keeps its bytes)
                    [&](const void* const* src, hipStream_t s) { return refit_mesh_one(mesh, (const float*)src[0], (const float*)src[1], s); });
}

int get_mesh_refit_info(ArtMeshRefitInfo* out) { return get_info(out, "null ArtMeshRefitInfo", g_mesh_refit_info, fold_mesh_refit); }

// ---- the two-level scene as it lies in HBM (art_export_two_level) -------------------------------------------------------------------
// Device 0's arrays, copied after its stream has drained (an update on another stream is ordered before the context stream's later
// work).  The per-mesh values: the plan's working buffer once an update has built the plan, the build's before that.
int export_two_level(ArtTwoLevelInfo* info, const ArtTwoLevelBuffers* buf) {
  const std::string name = "art_export_two_level";
  if (!info) return fail(name + ": null ArtTwoLevelInfo");
  Ctx& c = g_devs[0];
  if (!c.scene_ready) return fail(name + ": no scene uploaded");
  const HostScene& hs = c.host_scene;
  if (hs.gcore_seam) return fail(name + ": the scene was committed through gcore_commit_scene, which keeps its own two-level tree");
  if (c.scene.n_inst <= 0) return fail(name + ": the scene is not instanced (n_instances = 0); art_export_bvh exports the tree of a flat mesh");
  const TwoLevelHost& T = hs.two;
  const size_t n_entry = T.entry.size(), n_inst = T.inst.size(), nm = T.mesh_pad_abs.size(), n_tlas = (size_t)T.tlas.n_nodes;
  const size_t n_blas = T.blas_nodes.size() / 32, n_rec = T.blas_tris.size() / kTriFloats;
  if (!arrays_are_the_kept_builds(c, T)) return fail(name + ": internal: the arrays in HBM are not the kept build's");
  const Ctx::MovePlan& P = c.move;
  std::memset(info, 0, sizeof *info);
  info->n_inst = (int32_t)n_inst; info->n_entry = (int32_t)n_entry; info->n_mesh = (int32_t)nm; info->n_tlas_nodes = (int32_t)n_tlas;
  info->n_blas_nodes = (int32_t)n_blas; info->n_records = (int32_t)n_rec; info->inst_shift = c.scene.inst_shift; info->updated = P.ready ? 1 : 0;
  const BvhBuildParams tp;                                                 // (the instance tree builder's pad rule: build_move_plan)
  info->mesh_pad_rel = T.mesh_pad_rel; info->mesh_pad_min = T.mesh_pad_min; info->scene_extent = T.scene_extent;
  info->tlas_pad_rel = tp.inflate_rel; info->tlas_pad_abs = tp.inflate_abs;
  if (!buf) return 0;
  void* const dst[10] = {buf->inst, buf->tlas_nodes, buf->tlas_tris, buf->blas_nodes, buf->blas_tris, buf->qnodes, buf->mesh_pad, buf->mesh_box, buf->mesh_base, buf->node_mesh};
  const size_t words[10] = {n_entry * 32, n_tlas * 32, n_entry * kTriFloats, n_blas * 32, n_rec * kTriFloats, (n_tlas + n_blas) * 16, nm, 6 * nm, 3 * nm, n_blas};
  static const char* const what[10] = {"inst", "tlas_nodes", "tlas_tris", "blas_nodes", "blas_tris", "qnodes", "mesh_pad", "mesh_box", "mesh_base", "node_mesh"};
  bool any = false;
  for (int k = 0; k < 10; ++k) {
    if (!dst[k]) continue;
    any = true;
    if (buf->cap[k] < (int64_t)words[k]) return fail(name + ": buffer " + what[k] + " too small (" + std::to_string(words[k]) + " words)");
  }
  if (!any) return 0;
  MovePlanHost H;
  if (!P.ready && (dst[6] || dst[7] || dst[8] || dst[9])) {
    std::string err;
    if (!build_move_plan_host(T, H, err)) return fail(name + ": " + err);
  }
  Dev0Guard guard;
  if (use_dev(0)) return 1;
  HIP_TRY(hipStreamSynchronize(c.stream));
  const void* const dev[6] = {c.b_inst.p, c.b_tlas_nodes.p, c.b_tlas_tris.p, c.b_blas_nodes.p, c.b_blas_tris.p, c.b_qnodes.p};
  for (int k = 0; k < 6; ++k) if (dst[k] && words[k]) HIP_TRY(hipMemcpy(dst[k], dev[k], words[k] * 4, hipMemcpyDeviceToHost));
  const void* const plan_dev[4] = {P.args.pad_cur, P.args.mesh_box, P.args.mesh_base, P.args.node_mesh};
  const void* const plan_host[4] = {H.pad_abs.data(), H.mesh_box.data(), H.mesh_base.data(), H.node_mesh.data()};
  for (int k = 0; k < 4; ++k) {
    if (!dst[6 + k] || !words[6 + k]) continue;
    if (P.ready) HIP_TRY(hipMemcpy(dst[6 + k], plan_dev[k], words[6 + k] * 4, hipMemcpyDeviceToHost));
    else std::memcpy(dst[6 + k], plan_host[k], words[6 + k] * 4);
  }
  return 0;
}

// ---- replacing a tree: what art_rebuild_device, art_rebuild_instance_tree_device and art_rebuild_mesh_tree_device share -------------
// The rebuild waits for the host anyway: what the library's streams and the caller's stream hold is done before anything is built.
// qs: the caller's stream as device 0 names it.  Device 0 is current afterwards.
static int quiesce(hipStream_t st, hipStream_t& qs) {
  Ctx& c0 = g_devs[0];
  qs = StreamOrder(c0, st).qs;
  for (int k = 0; k < g_ndev; ++k) {
    if (use_dev(k)) return 1;
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  }
  if (use_dev(0)) return 1;
  if (qs != c0.stream) HIP_TRY(hipStreamSynchronize(qs));
  return 0;
}

// What the last update of an instanced scene left in force on device 0 (no plan: the upload's placement and records, which it checked).
// why: what that state denies the call, and what clears it.
static int refuse_bad_state(const std::string& name, const char* why) {
  const Ctx::MovePlan& P = g_devs[0].move;
  if (!P.ready) return 0;
  unsigned long long w[kMoveStateWords];
  HIP_TRY(hipMemcpy(w, P.args.state, sizeof w, hipMemcpyDeviceToHost));
  if (!w[1] && !w[7]) return 0;
  return fail(name + ": " + std::to_string(w[1]) + " bad instance matrix(es) and " + std::to_string(w[7]) + " bad vertex coordinate(s) are in force, " + std::to_string(w[1] + w[7]) + " in all: " + why);
}

// a build's counter words, once s is idle
template <int N>
static int read_counters(hipStream_t s, const unsigned long long* bad, unsigned long long (&w)[N]) {
  HIP_TRY(hipMemcpyAsync(w, bad, sizeof w, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

// The current context's gather on stream s: the counter words zeroed, `launch` between a pair of c.rebuild_pairs, the words read back
// (s is idle then) and the pair's time given to *gather_ms where the caller asks for it.  zeroed: a buffer the gather must find zeroed.
template <int N, typename Launch>
static int timed_gather(hipStream_t s, unsigned long long* bad, unsigned long long (&w)[N], float* gather_ms, Launch launch, const DevBuf* zeroed = nullptr) {
  Ctx& c = g_ctx;
  EventPairs::Timer timer;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof w, s));
  if (zeroed) HIP_TRY(hipMemsetAsync(zeroed->p, 0, zeroed->bytes, s));
  HIP_TRY(c.rebuild_pairs.begin(timer, s));
  launch();
  HIP_TRY(hipGetLastError());
  HIP_TRY(timer.end());
  if (read_counters(s, bad, w)) return 1;
  HIP_TRY(c.rebuild_pairs.fold(/*wait=*/true, [gather_ms](float ms, uint8_t) { if (gather_ms) *gather_ms = ms; }));      // (the last pair is this gather's)
  return 0;
}

// the scratch of one context's build in HBM, released on every way out of it
struct BuildScratch { DevBuf t9, bad, order, maps; ~BuildScratch() { t9.release(); bad.release(); order.release(); maps.release(); } };

// What one context has built and not yet committed: the builder's tree and the N buffers a kind names.  Whatever is still here when the
// call leaves is freed, so a rebuild that fails anywhere leaves every context's scene as it was.
template <int N>
struct Pending {
  int device = -1; GpuBvh g; DevBuf buf[N];
  Pending() = default;
  Pending(const Pending&) = delete;
  ~Pending() { if (device >= 0) (void)hipSetDevice(device); free_tree(g); for (DevBuf& b : buf) b.release(); }
};

// built buffers become the current context's: {mine, built} pairs
static void take_built(std::initializer_list<std::pair<DevBuf*, DevBuf*>> pairs) {
  for (const std::pair<DevBuf*, DevBuf*>& mb : pairs) { mb.first->release(); *mb.first = *mb.second; *mb.second = DevBuf(); }      // (owned by the context now)
}

// The driver of the three calls, after the kind's own refusals (t0: the call's first line).  Every context builds into new buffers
// before any context's scene changes: every check and allocation comes before the first swap, and a failure before it leaves every
// context as it was.  A failure after it means a lost device, the one case in which contexts may end up with different trees.
//   prepare(k)                       nothing is built yet: what the kind refuses in force, and context k's plan
//   build(k, s, pending, gather_ms)  context k's new tree on s (context 0: the caller's stream, and the gather time that is reported);
//                                    returns with s idle and has touched nothing of the context's scene or plan
//   fold()                           whatever else can fail without a lost device: context k's events and counters of the kind
//   before_commit(first)             what the commits take from the host
//   commit(pending)                  context k takes its tree.  No step allocates or waits for anything but its own copy; the one that
//                                    can fail, the copy of the new header to d_scene, comes first, while the buffers are the old ones
//   after(built, qs)                 the host's copies follow, and what the kind still enqueues on the new tree
// Context k is current in prepare, build, fold and commit.  A call is counted once all of it has succeeded.
template <typename P, typename Info, typename Prepare, typename Build, typename Fold, typename Before, typename Commit, typename After>
static int run_rebuild(std::chrono::steady_clock::time_point t0, hipStream_t st, Info& info, Prepare prepare, Build build, Fold fold, Before before_commit, Commit commit, After after) {
  Dev0Guard guard;
  hipStream_t qs = nullptr;
  if (use_dev(0) || quiesce(st, qs)) return 1;
  for (int k = 0; k < g_ndev; ++k) { if (use_dev(k) || prepare(k)) return 1; }
  std::vector<P> built((size_t)g_ndev);
  float gather_ms = 0.0f;
  for (int k = 0; k < g_ndev; ++k) {
    if (use_dev(k)) return 1;
    built[(size_t)k].device = g_ctx.device;
    if (build(k, k == 0 ? qs : g_ctx.stream, built[(size_t)k], k == 0 ? &gather_ms : nullptr)) return 1;
  }
  for (int k = 0; k < g_ndev; ++k) { if (use_dev(k) || fold()) return 1; }
  // ---- commit: from here on the scene changes
  before_commit(built[0]);
  for (int k = 0; k < g_ndev; ++k) { if (use_dev(k) || commit(built[(size_t)k])) return 1; }
  if (after(built, qs)) return 1;
  info.rebuilds += 1; info.gather_ms += gather_ms; info.build_ms += built[0].g.build_ms;
  info.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// the rebuild counts: cumulative since the upload, kept on the host (no stream is waited for)
template <typename Info>
static int get_rebuild_counts(Info* out, const char* null_msg, const Info& info) { if (!out) return fail(null_msg); *out = info; return 0; }

// what both rebuilds of an instanced scene prepare and fold
static int prepare_instanced(int k, const HostScene& hs, const std::string& name, const char* why) {
  double plan_ms = 0.0;                                                    // (no update has run yet: the plan's time is this call's host time)
  return (k == 0 && refuse_bad_state(name, why)) || (!g_ctx.move.ready && build_move_plan(hs, name, plan_ms));
}
static int fold_instanced() { return fold_move() || fold_mesh_refit(); }

// ---- a new tree from device-resident vertices (art_rebuild_device, art_rebuild.hip) -----------------------------------------------
struct PendingTree : Pending<3> {
  DevBuf& qtris() { return buf[0]; }
  DevBuf& idx() { return buf[1]; }             // the mesh's index triples where no refit plan held them (or, after the commit, the plan's)
  DevBuf& stage() { return buf[2]; }           // contexts k > 0: peer copy of pos (+ nrm)
};

// the current context's new tree on stream s, from positions in this context's device memory: gather, count the bad vertices, build,
// check, pad.  Returns with s idle.  Nothing of the context's scene is touched.
static int rebuild_one(const HostScene& hs, const BvhBuildParams& bp, const float* pos, hipStream_t s, PendingTree& out, float* gather_ms) {
  Ctx& c = g_ctx;
  const int32_t n_prims = (int32_t)(hs.m_idx.size() / 3);
  BuildScratch sc;
  const int32_t* idx = (const int32_t*)c.refit.b_idx.p;                   // the refit plan keeps the index triples in HBM
  if (!c.refit.ready || !idx) { if (upload(out.idx(), hs.m_idx)) return 1; idx = (const int32_t*)out.idx().p; }
  if (ensure(sc.t9, (size_t)n_prims * 9 * sizeof(float)) || ensure(sc.bad, sizeof(unsigned long long))) return 1;
  GatherArgs G;
  G.pos3f = pos; G.idx = idx; G.nverts = hs.m_nverts; G.n_prims = n_prims; G.tri9 = (float*)sc.t9.p; G.bad = (unsigned long long*)sc.bad.p;
  unsigned long long n_bad[1];
  if (timed_gather(s, G.bad, n_bad, gather_ms, [&] { launch_gather_tri9(s, G); })) return 1;
  if (n_bad[0]) return fail("art_rebuild_device: " + std::to_string(n_bad[0]) + " vertex coordinate(s) not finite or beyond 1e18 in magnitude; the tree was not rebuilt and the scene is unchanged");
  std::string err;
  if (!build_bvh8_gpu((const float*)sc.t9.p, n_prims, bp, s, out.g, err)) return fail("art_rebuild_device: GPU BVH build: " + err);
  if (check_tree_limits(bp.width, out.g.n_nodes, out.g.n_tris, true, true, out.g.qnodes != nullptr, out.g.max_stack)) return 1;
  if (bp.width == 4 && pad_tri_records(out.qtris(), out.g.tris, out.g.n_tris, s)) return 1;
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

// the current context takes its new tree (its streams are idle, its refit events are folded)
static int commit_tree(const BvhBuildParams& bp, PendingTree& t) {
  Ctx& c = g_ctx;
  {
    DevScene s = c.scene;
    s.nodes = t.g.nodes; s.tris = t.g.tris; s.n_nodes = t.g.n_nodes; s.n_tris = t.g.n_tris; s.node_width = bp.width;
    HIP_TRY(hipMemcpy(c.d_scene, &s, sizeof(DevScene), hipMemcpyHostToDevice));
  }
  if (!t.idx().p) { t.idx() = c.refit.b_idx; c.refit.b_idx = DevBuf(); }     // (kept for the shading records)
  release_updates(c);                                                     // the next refit plans against the new tree
  c.opt.bvh_params = g_devs[0].opt.bvh_params;                                    // (the options as they stand; bp may name builder 3 in place of 0)
  adopt_tree(c, t.g, bp.width);
  take_built({{&c.b_qtris, &t.qtris()}});
  DevScene& s = c.scene;
  s.nodes = (const float*)c.b_nodes.p; s.tris = (const float*)c.b_tris.p;
  s.n_nodes = t.g.n_nodes; s.n_tris = t.g.n_tris; s.node_width = bp.width;
  return 0;
}

int rebuild_device(const float* pos, const float* nrm, int64_t nverts, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  if (check_mesh_update(kRebuildCall, pos, nverts)) return 1;
  Ctx& c0 = g_devs[0];
  HostScene& hs = c0.host_scene;
  BvhBuildParams bp = c0.opt.bvh_params;
  if (bp.spatial_alpha >= 0.0f) return fail("art_rebuild_device: option bvh_spatial_splits is set; reference splitting exists in the host builder only (art_upload_scene builds that tree)");
  if (hs.m_idx.size() / 3 < 2) return fail("art_rebuild_device: a mesh of fewer than two triangles has no GPU-built tree; art_refit_device moves it");
  if (bp.builder == 0) bp.builder = 3;                                    // the host builder's tree, from the GPU binned-SAH builder
  const size_t bytes = 12 * (size_t)nverts;
  if (check_planes({{pos, bytes, "pos3f"}, {nrm, bytes, "nrm3f"}})) return 1;      // (against g_ctx: context 0, which every call leaves current)
  return run_rebuild<PendingTree>(t0, st, g_rebuild_info,
      [](int) { return 0; },
      [&](int k, hipStream_t s, PendingTree& t, float* gather_ms) {
        const float* p = pos;
        if (k > 0) {
          const int dev = g_ctx.device;
          if (ensure(t.stage(), nrm ? 2 * bytes : bytes)) return 1;
          float* sp = (float*)t.stage().p;
          if (hipMemcpyPeer(sp, dev, pos, c0.device, bytes) != hipSuccess || (nrm && hipMemcpyPeer(sp + 3 * (size_t)nverts, dev, nrm, c0.device, bytes) != hipSuccess))
            return fail("art_rebuild_device: copy to device " + std::to_string(dev) + " failed");
          p = sp;
        }
        return rebuild_one(hs, bp, p, s, t, gather_ms);
      },
      fold_refit,
      [](const PendingTree&) {},
      [&](PendingTree& t) { return commit_tree(bp, t); },
      [&](std::vector<PendingTree>& built, hipStream_t qs) {
        const GpuBvh& g = built[0].g;
        hs.hdr.n_nodes = g.n_nodes; hs.hdr.n_tris = g.n_tris; hs.hdr.node_width = bp.width;
        hs.bvh.width = bp.width; hs.bvh.n_nodes = g.n_nodes; hs.bvh.n_tris = g.n_tris; hs.bvh.max_stack = g.max_stack;
        hs.bvh_build_ms = g.build_ms; hs.gpu_built = true; hs.refitted = false;
        drop_stale_host_copies(hs);
        for (int k = 0; k < g_ndev && nrm; ++k) {                         // the shading records: k_refit_tris' normals branch, no triangle records (n_recs = 0)
          if (use_dev(k)) return 1;
          Ctx& c = g_ctx;
          const hipStream_t s = (k == 0) ? qs : c.stream;
          const float* n = (k == 0) ? nrm : (const float*)built[(size_t)k].stage().p + 3 * (size_t)nverts;
          RefitArgs A;
          std::memset(&A, 0, sizeof A);
          A.nrm3f = n; A.idx = (const int32_t*)built[(size_t)k].idx().p; A.n_prims = (int32_t)(hs.m_idx.size() / 3); A.m_shade = (float*)c.b_m_shade.p;
          hs.m_shade_stale = true;                                        // (art_trace_rays reads the shading records on the host)
          launch_refit_tris(s, A);
          if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("art_rebuild_device: rewriting the shading records failed");
        }
        return 0;
      });
}

int get_rebuild_info(ArtRebuildInfo* out) { return get_rebuild_counts(out, "null ArtRebuildInfo", g_rebuild_info); }

// ---- a new instance tree from the proxy records in HBM (art_rebuild_instance_tree_device, art_move.hip + art_sah.hip) ---------------
struct PendingInstTree : Pending<5> {
  DevBuf& nodes() { return buf[0]; } DevBuf& tris() { return buf[1]; } DevBuf& qnodes() { return buf[2]; } DevBuf& inst() { return buf[3]; }      // the new instance tree's packets and proxy records, the new merged node array, the new instance table
  DevBuf& plan() { return buf[4]; }            // the plan's parts that follow the instance tree (Ctx::MovePlan::b_tlas)
  size_t o_lev = 0, o_prox = 0, o_mbase = 0, o_tight = 0;
  std::vector<int> level_off;
  int32_t n_tlas = 0, max_stack = 0;
};

// The built tree's packets and records as read back (the builder's numbering; word 9 of a record = the index of its proxy in `order`),
// checked as build_move_plan_host checks a build -- every node reached exactly once, every entry point named by exactly one proxy -- and
// re-planned: the host builder's numbering and the levels in that numbering (renumber_built_tree, art_renumber.h, which states the rule
// and serves a mesh's tree with its leaves of up to kMaxLeafTris records as well), and proxy_rec.
static bool plan_built_tree(const std::vector<float>& nodes, const std::vector<float>& tris, const std::vector<int32_t>& order, std::vector<int32_t>& node_map,
                            std::vector<int32_t>& rec_map, std::vector<int32_t>& levels, std::vector<int>& level_off, std::vector<int32_t>& proxy_rec, std::string& err) {
  const int64_t N = (int64_t)(nodes.size() / 32), n_entry = (int64_t)order.size();
  if (!renumber_built_tree(nodes.data(), N, n_entry, /*max_leaf=*/1, "instance tree", node_map, rec_map, levels, level_off, err)) return false;
  proxy_rec.assign((size_t)n_entry, -1);
  for (int64_t r = 0; r < n_entry; ++r) {
    int32_t idx;
    std::memcpy(&idx, &tris[(size_t)r * kTriFloats + 9], 4);
    if (idx < 0 || idx >= n_entry || proxy_rec[(size_t)order[(size_t)idx]] >= 0) { err = "a proxy of the built instance tree names no entry point, or one twice"; return false; }
    proxy_rec[(size_t)order[(size_t)idx]] = rec_map[(size_t)r];
  }
  return true;
}

// the current context's new instance tree on stream s: gather, count the proxies without a box, build, read back, check and re-plan,
// renumber, relocate.  Returns with s idle.  Nothing of the context's scene or plan is touched.
static int rebuild_inst_one(const std::vector<int32_t>& order, hipStream_t s, PendingInstTree& out, float* gather_ms) {
  const std::string name = "art_rebuild_instance_tree_device";
  Ctx& c = g_ctx;
  const Ctx::MovePlan& P = c.move;
  const int32_t n_entry = P.args.n_entry, n_blas = P.args.n_blas_nodes, nm = P.args.n_mesh;
  BuildScratch sc;
  if (upload(sc.order, order) || ensure(sc.t9, (size_t)n_entry * 9 * sizeof(float)) || ensure(sc.bad, 2 * sizeof(unsigned long long))) return 1;
  InstRebuildArgs R;
  std::memset(&R, 0, sizeof R);
  R.n_entry = n_entry; R.n_blas_nodes = n_blas; R.n_tlas_old = P.n_tlas;
  R.order = (const int32_t*)sc.order.p; R.proxy_rec = P.args.proxy_rec; R.tlas_tris = P.args.tlas_tris;
  R.tri9 = (float*)sc.t9.p; R.bad = (unsigned long long*)sc.bad.p;
  unsigned long long n_bad[2];
  if (timed_gather(s, R.bad, n_bad, gather_ms, [&] { launch_inst_gather(s, R); })) return 1;
  if (n_bad[0]) return fail(name + ": " + std::to_string(n_bad[0]) + " entry point(s) without a finite world box; the tree was not rebuilt and the scene is unchanged");
  BvhBuildParams tp; tp.width = 4; tp.max_leaf = 1;                        // what build_two_level_host gives the instance tree
  std::string err;
  if (!build_bvh_sah_gpu((const float*)sc.t9.p, n_entry, tp, s, out.g, err)) return fail(name + ": GPU BVH build: " + err);
  const int32_t n_new = out.g.n_nodes;
  if (!out.g.qnodes || n_new < 1 || out.g.n_tris != n_entry) return fail(name + ": internal: the GPU build returned no instance tree");
  if (out.g.max_stack > kInstTopStack) return fail(name + ": instance tree stack bound " + std::to_string(out.g.max_stack) + " exceeds " + std::to_string(kInstTopStack));
  if (((size_t)n_new + (size_t)n_blas) * kQNodeBytes >= (1ull << 31)) return fail(name + ": instanced scene too large for 31-bit node offsets");
  std::vector<float> h_nodes((size_t)n_new * 32), h_tris((size_t)n_entry * kTriFloats);
  HIP_TRY(hipMemcpy(h_nodes.data(), out.g.nodes, h_nodes.size() * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_tris.data(), out.g.tris, h_tris.size() * 4, hipMemcpyDeviceToHost));
  std::vector<int32_t> node_map, rec_map, levels, proxy_rec, mesh_base((size_t)3 * (size_t)nm);
  if (!plan_built_tree(h_nodes, h_tris, order, node_map, rec_map, levels, out.level_off, proxy_rec, err)) return fail(name + ": internal: " + err);
  HIP_TRY(hipMemcpy(mesh_base.data(), P.args.mesh_base, mesh_base.size() * 4, hipMemcpyDeviceToHost));
  for (int32_t m = 0; m < nm; ++m) mesh_base[3 * (size_t)m + 2] += n_new - P.n_tlas;                       // (first node in qnodes)
  PlanImage img;
  out.o_lev = img.put(levels.data(), levels.size() * 4); out.o_prox = img.put(proxy_rec.data(), proxy_rec.size() * 4); out.o_mbase = img.put(mesh_base.data(), mesh_base.size() * 4);
  out.o_tight = img.put(nullptr, (size_t)n_new * 24);                      // (scratch: every level writes a node's tight box before the level above reads it)
  node_map.insert(node_map.end(), rec_map.begin(), rec_map.end());
  if (img.upload_to(out.plan()) || upload(sc.maps, node_map)) return 1;
  if (ensure(out.nodes(), (size_t)n_new * 128) || ensure(out.tris(), (size_t)n_entry * kTriBytes) || ensure(out.qnodes(), ((size_t)n_new + (size_t)n_blas) * kQNodeBytes) ||
      ensure(out.inst(), (size_t)n_entry * sizeof(DevInstance))) return 1;
  R.n_tlas_new = n_new;
  R.g_nodes = out.g.nodes; R.g_tris = out.g.tris; R.g_qnodes = (const QNode*)out.g.qnodes;
  R.node_map = (const int32_t*)sc.maps.p; R.rec_map = (const int32_t*)sc.maps.p + n_new;
  R.nodes_out = (float*)out.nodes().p; R.tris_out = (float*)out.tris().p;
  R.qnodes_old = (const QNode*)c.b_qnodes.p; R.qnodes_out = (QNode*)out.qnodes().p;
  R.inst_old = (const DevInstance*)c.b_inst.p; R.inst_out = (DevInstance*)out.inst().p;
  launch_inst_finish(s, R);
  launch_inst_relocate(s, R);
  HIP_TRY(hipGetLastError());
  if (read_counters(s, R.bad, n_bad)) return 1;
  if (n_bad[1]) return fail(name + ": internal: " + std::to_string(n_bad[1]) + " leaf(s) of the built instance tree refused");
  free_tree(out.g);                                                        // (the renumbered copy is the tree)
  out.n_tlas = n_new; out.max_stack = out.g.max_stack;
  return 0;
}

// the current context takes its new instance tree (its streams are idle, its move events are folded)
static int commit_inst_tree(const HostScene& hs, PendingInstTree& t) {
  Ctx& c = g_ctx;
  DevScene s = c.scene;
  s.inst = (const DevInstance*)t.inst().p; s.tlas_nodes = (const float*)t.nodes().p; s.tlas_tris = (const float*)t.tris().p; s.n_nodes = t.n_tlas;
  HIP_TRY(hipMemcpy(c.d_scene, &s, sizeof(DevScene), hipMemcpyHostToDevice));
  c.scene = s;
  Ctx::MovePlan& P = c.move;
  take_built({{&c.b_inst, &t.inst()}, {&c.b_tlas_nodes, &t.nodes()}, {&c.b_tlas_tris, &t.tris()}, {&c.b_qnodes, &t.qnodes()}, {&P.b_tlas, &t.plan()}});
  const char* pb = (const char*)P.b_tlas.p;
  MoveArgs& A = P.args;
  A.inst = (DevInstance*)c.b_inst.p; A.tlas_nodes = (float*)c.b_tlas_nodes.p; A.tlas_tris = (float*)c.b_tlas_tris.p; A.qnodes = (QNode*)c.b_qnodes.p;
  A.proxy_rec = (const int32_t*)(pb + t.o_prox); A.mesh_base = (const int32_t*)(pb + t.o_mbase); A.tlas_tight = (float*)(pb + t.o_tight);
  P.levels = (const int32_t*)(pb + t.o_lev); P.level_off = t.level_off; P.n_tlas = t.n_tlas;
  c.bvh_stack_bound = std::max(8, t.max_stack + 3 + hs.two.blas_max_stack);      // (flatten_scene's bound: both trees and the "leave" marker on one stack)
  c.blocks_per_cu = 0;   // re-query occupancy
  return 0;
}

// every context builds from its own proxy records
int rebuild_instance_tree_device(hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  const std::string name = "art_rebuild_instance_tree_device";
  Ctx& c0 = g_devs[0];
  if (!c0.scene_ready) return fail(name + ": no scene uploaded");
  HostScene& hs = c0.host_scene;
  if (hs.gcore_seam) return fail(name + ": the scene was committed through gcore_commit_scene, which keeps its own two-level tree");
  if (c0.scene.n_inst <= 0) return fail(name + ": the scene is not instanced (n_instances = 0); art_rebuild_device builds the tree of a flat mesh");
  const size_t n_entry = hs.two.entry.size();
  if (n_entry < 2) return fail(name + ": an instance tree over fewer than two entry points has nothing to rebuild");
  std::vector<int32_t> order(n_entry);                                    // the upload's proxy order: entry points by (instance, root_entry)
  for (size_t e = 0; e < n_entry; ++e) order[e] = (int32_t)e;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    const TwoLevelHost::EntryPoint &x = hs.two.entry[(size_t)a], &y = hs.two.entry[(size_t)b];
    return x.inst < y.inst || (x.inst == y.inst && x.root_entry < y.root_entry);
  });
  return run_rebuild<PendingInstTree>(t0, st, g_inst_rebuild_info,
      [&](int k) { return prepare_instanced(k, hs, name, "their entry points have no box to build over; a good art_move_instances_device or art_refit_mesh_device clears that state"); },
      [&](int, hipStream_t s, PendingInstTree& t, float* gather_ms) { return rebuild_inst_one(order, s, t, gather_ms); },
      fold_instanced,
      [](const PendingInstTree&) {},
      [&](PendingInstTree& t) { return commit_inst_tree(hs, t); },
      [&](std::vector<PendingInstTree>& built, hipStream_t) {
        // the host's copies: the sizes follow; the tree's arrays in hs.two have been stale since the first update, the table's qroot words go stale now
        const int32_t n_new = built[0].n_tlas, max_stack = built[0].max_stack, shift = n_new - hs.two.tlas.n_nodes;
        hs.two.tlas.n_nodes = n_new; hs.two.tlas.max_stack = max_stack;
        for (int32_t& b : hs.two.qnode_base) b += shift;
        hs.hdr.n_nodes = n_new; hs.bvh.n_nodes += shift; hs.bvh.max_stack = std::max(max_stack + 3 + hs.two.blas_max_stack, 8);
        hs.inst_stale = true;
        return 0;
      });
}

int get_instance_rebuild_info(ArtInstanceRebuildInfo* out) { return get_rebuild_counts(out, "null ArtInstanceRebuildInfo", g_inst_rebuild_info); }

// ---- a new tree for one mesh from its triangle records in HBM (art_rebuild_mesh_tree_device, art_move.hip + art_sah.hip) -------------
struct PendingMeshTree : Pending<6> {
  DevBuf& nodes() { return buf[0]; } DevBuf& tris() { return buf[1]; } DevBuf& qtris() { return buf[2]; } DevBuf& qnodes() { return buf[3]; } DevBuf& inst() { return buf[4]; }      // the new blas_nodes, blas_tris and padded copy, the new merged node array, the new instance table
  DevBuf& plan() { return buf[5]; }            // the plan's parts that follow the meshes' node layout (Ctx::MovePlan::b_blas)
  size_t o_mbase = 0, o_lev = 0, o_nmesh = 0, o_tight = 0;
  std::vector<int> level_off;                  // the new blas_level_off
  std::vector<int> mesh_level_first;           // per mesh, and one past the last: its levels in level_off
  int32_t n_blas = 0, max_stack = 0;
};

// the current context's new tree of mesh `mesh` on stream s: gather, count the bad records, build, read back, check and renumber, finish,
// relocate, tight boxes.  Returns with s idle.  Nothing of the context's scene or plan is touched.
static int rebuild_mesh_one(const HostScene& hs, int32_t mesh, hipStream_t s, PendingMeshTree& out, float* gather_ms) {
  const std::string name = "art_rebuild_mesh_tree_device";
  Ctx& c = g_ctx;
  const Ctx::MovePlan& P = c.move;
  const Ctx::MovePlan::Mesh& M = P.meshes[(size_t)mesh];
  const int32_t nm = P.args.n_mesh, n_blas = P.args.n_blas_nodes, n_entry = P.args.n_entry, n_recs = M.n_recs;
  BuildScratch sc;
  std::vector<int32_t> mesh_base((size_t)3 * (size_t)nm), old_levels((size_t)n_blas);
  float pad = 0.0f;
  HIP_TRY(hipMemcpy(mesh_base.data(), P.args.mesh_base, mesh_base.size() * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(old_levels.data(), P.blas_levels, old_levels.size() * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&pad, P.args.pad_cur + mesh, 4, hipMemcpyDeviceToHost));   // the pad the mesh carries now: pads only grow, and the new boxes must not be tighter than a move has asked for
  MeshRebuildArgs R;
  std::memset(&R, 0, sizeof R);
  R.mesh = mesh; R.n_recs = n_recs;
  R.nb = mesh_base[3 * (size_t)mesh]; R.tb = mesh_base[3 * (size_t)mesh + 1]; R.qb = mesh_base[3 * (size_t)mesh + 2];
  R.n_old = ((mesh + 1 < nm) ? mesh_base[3 * ((size_t)mesh + 1)] : n_blas) - R.nb;
  R.n_tlas = P.n_tlas; R.n_blas_old = n_blas; R.n_entry = n_entry;
  if (R.nb < 0 || R.n_old < 1 || R.nb + R.n_old > n_blas || R.tb != M.tri_base || R.qb != R.n_tlas + R.nb || n_recs != M.n_prims || c.b_blas_nodes.bytes != (size_t)n_blas * 128 ||
      c.b_qnodes.bytes != ((size_t)R.n_tlas + (size_t)n_blas) * kQNodeBytes || (size_t)(R.tb + n_recs) * kTriBytes > c.b_blas_tris.bytes)
    return fail(name + ": internal: the plan is not the layout in HBM");
  if (ensure(sc.t9, (size_t)n_recs * 9 * sizeof(float)) || ensure(sc.bad, 2 * sizeof(unsigned long long))) return 1;
  R.tris_old = (const float*)c.b_blas_tris.p; R.tri9 = (float*)sc.t9.p; R.bad = (unsigned long long*)sc.bad.p;
  unsigned long long n_bad[2];
  if (timed_gather(s, R.bad, n_bad, gather_ms, [&] { launch_mesh_gather(s, R); }, &sc.t9)) return 1;      // (t9 zeroed: an index named twice leaves a triangle unwritten, a defined input, which the checks below then refuse or not)
  if (n_bad[0]) return fail(name + ": " + std::to_string(n_bad[0]) + " triangle record(s) of mesh " + std::to_string(mesh) + " with an index out of range or a corner that is not finite; the tree was not rebuilt and the scene is unchanged");
  BvhBuildParams bp; bp.width = 4;                                         // what build_two_level_host gives a mesh of a one-sided build, at the pad in force
  bp.inflate_rel = hs.two.mesh_pad_rel; bp.inflate_abs = pad;
  std::string err;
  if (!build_bvh_sah_gpu((const float*)sc.t9.p, n_recs, bp, s, out.g, err)) return fail(name + ": GPU BVH build: " + err);
  const int32_t n_new = out.g.n_nodes;
  if (!out.g.qnodes || n_new < 1 || out.g.n_tris != n_recs) return fail(name + ": internal: the GPU build returned no tree for the mesh");
  if (out.g.max_stack > kStackEntries) return fail(name + ": mesh tree stack bound " + std::to_string(out.g.max_stack) + " exceeds " + std::to_string(kStackEntries));
  const int64_t n_blas_new = (int64_t)n_blas - R.n_old + n_new;
  if (((uint64_t)R.n_tlas + (uint64_t)n_blas_new) * kQNodeBytes >= (1ull << 31)) return fail(name + ": instanced scene too large for 31-bit node offsets");
  std::vector<float> h_nodes((size_t)n_new * 32);
  HIP_TRY(hipMemcpy(h_nodes.data(), out.g.nodes, h_nodes.size() * 4, hipMemcpyDeviceToHost));
  std::vector<int32_t> node_map, rec_map, levels;
  std::vector<int> level_off;
  if (!renumber_built_tree(h_nodes.data(), n_new, n_recs, /*max_leaf=*/4, "mesh tree", node_map, rec_map, levels, level_off, err)) return fail(name + ": internal: " + err);
  R.n_new = n_new; R.delta = n_new - R.n_old;
  // the plan's parts that follow the node layout: mesh_base, and the level lists with this mesh's levels replaced and the meshes' behind it moved
  for (int32_t k = mesh + 1; k < nm; ++k) { mesh_base[3 * (size_t)k] += R.delta; mesh_base[3 * (size_t)k + 2] += R.delta; }
  std::vector<int32_t> new_levels;
  new_levels.reserve((size_t)n_blas_new);
  out.level_off.assign(1, 0); out.mesh_level_first.assign(1, 0);
  for (int32_t k = 0; k < nm; ++k) {
    if (k == mesh) {
      for (size_t L = 0; L + 1 < level_off.size(); ++L) {
        for (int i = level_off[L]; i < level_off[L + 1]; ++i) new_levels.push_back(R.nb + levels[(size_t)i]);
        out.level_off.push_back((int)new_levels.size());
      }
    } else {
      const Ctx::MovePlan::Mesh& K = P.meshes[(size_t)k];
      for (int L = K.level_first; L < K.level_end; ++L) {
        for (int i = P.blas_level_off[(size_t)L]; i < P.blas_level_off[(size_t)L + 1]; ++i) new_levels.push_back(old_levels[(size_t)i] + (k > mesh ? R.delta : 0));
        out.level_off.push_back((int)new_levels.size());
      }
    }
    out.mesh_level_first.push_back((int)out.level_off.size() - 1);
  }
  if ((int64_t)new_levels.size() != n_blas_new) return fail(name + ": internal: the plan's levels do not cover the meshes' nodes");
  PlanImage img;
  out.o_mbase = img.put(mesh_base.data(), mesh_base.size() * 4); out.o_lev = img.put(new_levels.data(), new_levels.size() * 4);
  out.o_nmesh = img.put(nullptr, (size_t)n_blas_new * 4); out.o_tight = img.put(nullptr, (size_t)n_blas_new * 24);      // (written by the finish, the relocation and the tight-box launches)
  node_map.insert(node_map.end(), rec_map.begin(), rec_map.end());
  if (img.upload_to(out.plan()) || upload(sc.maps, node_map)) return 1;
  if (ensure(out.nodes(), (size_t)n_blas_new * 128) || ensure(out.tris(), c.b_blas_tris.bytes) || ensure(out.qtris(), c.b_qtris.bytes) ||
      ensure(out.qnodes(), ((size_t)R.n_tlas + (size_t)n_blas_new) * kQNodeBytes) || ensure(out.inst(), (size_t)n_entry * sizeof(DevInstance))) return 1;
  char* pb = (char*)out.plan().p;
  R.g_nodes = out.g.nodes; R.g_tris = out.g.tris; R.g_qnodes = (const QNode*)out.g.qnodes;
  R.node_map = (const int32_t*)sc.maps.p; R.rec_map = (const int32_t*)sc.maps.p + n_new;
  R.nodes_out = (float*)out.nodes().p; R.tris_out = (float*)out.tris().p; R.qtris_out = (float*)out.qtris().p; R.qnodes_out = (QNode*)out.qnodes().p;
  R.node_mesh_out = (int32_t*)(pb + out.o_nmesh); R.tight_out = (float*)(pb + out.o_tight);
  R.nodes_old = (const float*)c.b_blas_nodes.p; R.qnodes_old = (const QNode*)c.b_qnodes.p; R.node_mesh_old = P.args.node_mesh; R.tight_old = P.args.blas_tight;
  R.inst_old = (const DevInstance*)c.b_inst.p; R.inst_out = (DevInstance*)out.inst().p; R.inst_mesh = P.args.inst_mesh;
  // record positions do not move: the other meshes' records and padded copies are plain copies, the finish then writes this mesh's slices
  HIP_TRY(hipMemcpyAsync(out.tris().p, c.b_blas_tris.p, c.b_blas_tris.bytes, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(out.qtris().p, c.b_qtris.p, c.b_qtris.bytes, hipMemcpyDeviceToDevice, s));
  launch_mesh_finish(s, R);
  launch_mesh_relocate(s, R);
  const int32_t* d_levels = (const int32_t*)(pb + out.o_lev);
  for (int L = out.mesh_level_first[(size_t)mesh + 1] - 1; L >= out.mesh_level_first[(size_t)mesh]; --L)      // deepest level first
    launch_mesh_tight_level(s, R, d_levels + out.level_off[(size_t)L], out.level_off[(size_t)L + 1] - out.level_off[(size_t)L]);
  HIP_TRY(hipGetLastError());
  if (read_counters(s, R.bad, n_bad)) return 1;
  if (n_bad[1]) return fail(name + ": internal: " + std::to_string(n_bad[1]) + " leaf(s) of the built mesh tree refused");
  free_tree(out.g);                                                        // (the renumbered copy is the tree)
  out.n_blas = (int32_t)n_blas_new; out.max_stack = out.g.max_stack;
  return 0;
}

// The current context takes its mesh's new tree (its streams are idle, its update events are folded).  The plan keeps everything its
// kernels maintain in b_work.
static int commit_mesh_tree(PendingMeshTree& t, int tlas_stack, int blas_stack) {
  Ctx& c = g_ctx;
  DevScene s = c.scene;
  s.inst = (const DevInstance*)t.inst().p; s.blas_nodes = (const float*)t.nodes().p; s.blas_tris = (const float*)t.tris().p;
  HIP_TRY(hipMemcpy(c.d_scene, &s, sizeof(DevScene), hipMemcpyHostToDevice));
  c.scene = s;
  Ctx::MovePlan& P = c.move;
  take_built({{&c.b_inst, &t.inst()}, {&c.b_blas_nodes, &t.nodes()}, {&c.b_blas_tris, &t.tris()}, {&c.b_qtris, &t.qtris()}, {&c.b_qnodes, &t.qnodes()}, {&P.b_blas, &t.plan()}});
  const char* pb = (const char*)P.b_blas.p;
  MoveArgs& A = P.args;
  A.inst = (DevInstance*)c.b_inst.p; A.blas_nodes = (float*)c.b_blas_nodes.p; A.blas_tris = (const float*)c.b_blas_tris.p; A.qnodes = (QNode*)c.b_qnodes.p;
  A.n_blas_nodes = t.n_blas;
  A.mesh_base = (const int32_t*)(pb + t.o_mbase); A.node_mesh = (const int32_t*)(pb + t.o_nmesh); A.blas_tight = (float*)(pb + t.o_tight);
  P.blas_levels = (const int32_t*)(pb + t.o_lev); P.blas_level_off = t.level_off;
  for (size_t k = 0; k < P.meshes.size(); ++k) { P.meshes[k].level_first = t.mesh_level_first[k]; P.meshes[k].level_end = t.mesh_level_first[k + 1]; }
  c.bvh_stack_bound = std::max(8, tlas_stack + 3 + blas_stack);           // (flatten_scene's bound: both trees and the "leave" marker on one stack)
  c.blocks_per_cu = 0;   // re-query occupancy
  return 0;
}

// the refusals art_rebuild_mesh_tree_device and art_get_mesh_tree_cost share
static int check_mesh_of_instanced(const std::string& name, int32_t mesh) {
  const Ctx& c0 = g_devs[0];
  if (!c0.scene_ready) return fail(name + ": no scene uploaded");
  const HostScene& hs = c0.host_scene;
  if (hs.gcore_seam) return fail(name + ": the scene was committed through gcore_commit_scene, which keeps its own two-level tree");
  if (c0.scene.n_inst <= 0) return fail(name + ": the scene is not instanced (n_instances = 0); " + (name == "art_get_mesh_tree_cost" ? "art_get_tree_cost has the figure of" : "art_rebuild_device builds the tree of") + " a flat mesh");
  const int64_t n_mesh = (int64_t)hs.mesh_nverts.size();
  if (mesh < 0 || mesh >= n_mesh || hs.mesh_idx_off.size() != (size_t)n_mesh + 1 || hs.two.qnode_base.size() != (size_t)n_mesh)
    return fail(name + ": mesh " + std::to_string(mesh) + " is out of range (the scene has " + std::to_string(n_mesh) + " meshes)");
  const int64_t n_tris = (hs.mesh_idx_off[(size_t)mesh + 1] - hs.mesh_idx_off[(size_t)mesh]) / 3;
  if (n_tris == 0) return fail(name + ": no instance shows mesh " + std::to_string(mesh));
  if (n_tris < 2) return fail(name + ": a mesh of fewer than two triangles has no GPU-built tree; art_refit_mesh_device moves it");
  return 0;
}

// every context builds from its own records
int rebuild_mesh_tree_device(int32_t mesh, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  const std::string name = "art_rebuild_mesh_tree_device";
  if (check_mesh_of_instanced(name, mesh)) return 1;
  Ctx& c0 = g_devs[0];
  HostScene& hs = c0.host_scene;
  for (size_t e = 0; e < hs.two.entry.size(); ++e) {
    const TwoLevelHost::EntryPoint& E = hs.two.entry[e];
    if (hs.two.inst[(size_t)E.inst].mesh == mesh && E.root_entry != 0)
      return fail(name + ": instance " + std::to_string(E.inst) + " of mesh " + std::to_string(mesh) + " was opened by the build (option inst_open): its entry points name subtrees of the "
                  "tree in force, and opening it again would change the instance table and the instance tree; art_upload_scene rebuilds such a mesh");
  }
  int32_t delta = 0;                                                       // the meshes' nodes: new count less old
  return run_rebuild<PendingMeshTree>(t0, st, g_mesh_rebuild_info,
      [&](int k) { return prepare_instanced(k, hs, name, "their boxes are empty and the plan's boxes do not describe the records; a good art_move_instances_device or art_refit_mesh_device clears that state"); },
      [&](int, hipStream_t s, PendingMeshTree& t, float* gather_ms) { return rebuild_mesh_one(hs, mesh, s, t, gather_ms); },
      fold_instanced,
      [&](const PendingMeshTree& first) {
        delta = first.n_blas - c0.move.args.n_blas_nodes;
        if (hs.two.mesh_max_stack.size() != hs.two.qnode_base.size()) hs.two.mesh_max_stack.assign(hs.two.qnode_base.size(), hs.two.blas_max_stack);
        hs.two.mesh_max_stack[(size_t)mesh] = first.max_stack;
        hs.two.blas_max_stack = *std::max_element(hs.two.mesh_max_stack.begin(), hs.two.mesh_max_stack.end());
      },
      [&](PendingMeshTree& t) { return commit_mesh_tree(t, hs.two.tlas.max_stack, hs.two.blas_max_stack); },
      [&](std::vector<PendingMeshTree>& built, hipStream_t) {
        // the host's copies: the sizes follow; the trees' arrays in hs.two have been stale since the first update, the table's node_base and qroot words go stale now
        for (size_t k = (size_t)mesh + 1; k < hs.two.qnode_base.size(); ++k) hs.two.qnode_base[k] += delta;
        for (InstRec& r : hs.two.inst) if (r.mesh > mesh) r.node_base += delta;
        hs.two.blas_nodes.resize((size_t)built[0].n_blas * 32, 0.0f); std::vector<uint32_t>().swap(hs.two.qnodes);
        hs.bvh.n_nodes += delta; hs.bvh.max_stack = std::max(hs.two.tlas.max_stack + 3 + hs.two.blas_max_stack, 8);
        hs.inst_stale = true;
        return 0;
      });
}

int get_mesh_rebuild_info(ArtMeshRebuildInfo* out) { return get_rebuild_counts(out, "null ArtMeshRebuildInfo", g_mesh_rebuild_info); }

// the cost figure of a tree of device 0 as it lies in HBM (an update on another stream is ordered before the context stream's later work)
static int tree_cost_of(Ctx& c, const float* nodes, int n_nodes, int width, ArtTreeCost* out) {
  Dev0Guard guard;
  if (use_dev(0)) return 1;
  DevBuf sums;
  struct Free { DevBuf& b; ~Free() { b.release(); } } fr{sums};
  if (ensure(sums, 4 * sizeof(double))) return 1;
  double h[4] = {0.0, 0.0, 0.0, 0.0};
  HIP_TRY(hipMemsetAsync(sums.p, 0, sizeof h, c.stream));
  launch_tree_cost(c.stream, nodes, n_nodes, width, (double*)sums.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h, sums.p, sizeof h, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  out->root_area = h[3];
  const bool any = h[3] > 0.0;                                            // (no usable child box under the root: no ray enters the tree)
  out->node_visits = 1.0 + (any ? h[0] / h[3] : 0.0);
  out->leaf_visits = any ? h[1] / h[3] : 0.0;
  out->tri_tests = any ? h[2] / h[3] : 0.0;
  return 0;
}

int get_tree_cost(ArtTreeCost* out) {
  if (!out) return fail("null ArtTreeCost");
  Ctx& c = g_devs[0];
  if (!c.scene_ready) return fail("art_get_tree_cost: no scene uploaded");
  if (c.scene.n_inst > 0) return fail("art_get_tree_cost: the scene is instanced (n_instances > 0); the figure is defined for the tree of a flat CLOSEST mesh");
  if (c.scene.n_nodes < 1 || !c.b_nodes.p) return fail("art_get_tree_cost: the scene has no tree (no ART_MESH_CLOSEST mesh)");
  return tree_cost_of(c, (const float*)c.b_nodes.p, c.scene.n_nodes, c.scene.node_width, out);
}

// the instance tree's packets: the same figure, a leaf slot being an entry point
int get_instance_tree_cost(ArtTreeCost* out) {
  if (!out) return fail("null ArtTreeCost");
  Ctx& c = g_devs[0];
  if (!c.scene_ready) return fail("art_get_instance_tree_cost: no scene uploaded");
  if (c.host_scene.gcore_seam) return fail("art_get_instance_tree_cost: the scene was committed through gcore_commit_scene, which keeps its own two-level tree");
  if (c.scene.n_inst <= 0) return fail("art_get_instance_tree_cost: the scene is not instanced (n_instances = 0); art_get_tree_cost has the figure of a flat mesh's tree");
  const int n_tlas = c.host_scene.two.tlas.n_nodes;
  if (n_tlas < 1 || c.b_tlas_nodes.bytes != (size_t)n_tlas * 128) return fail("art_get_instance_tree_cost: internal: the instance tree in HBM is not the kept build's");
  return tree_cost_of(c, (const float*)c.b_tlas_nodes.p, n_tlas, 4, out);
}

// one mesh's tree of an instanced scene: the same figure over its slice of blas_nodes, in object space
int get_mesh_tree_cost(int32_t mesh, ArtTreeCost* out) {
  if (!out) return fail("null ArtTreeCost");
  if (check_mesh_of_instanced("art_get_mesh_tree_cost", mesh)) return 1;
  Ctx& c = g_devs[0];
  const TwoLevelHost& T = c.host_scene.two;
  const int64_t n_blas = (int64_t)(c.b_blas_nodes.bytes / 128), nb = (int64_t)T.qnode_base[(size_t)mesh] - T.tlas.n_nodes;
  const int64_t ne = ((size_t)mesh + 1 < T.qnode_base.size()) ? (int64_t)T.qnode_base[(size_t)mesh + 1] - T.tlas.n_nodes : n_blas;
  if (nb < 0 || ne <= nb || ne > n_blas) return fail("art_get_mesh_tree_cost: internal: the meshes' trees in HBM are not the kept layout");
  return tree_cost_of(c, (const float*)c.b_blas_nodes.p + (size_t)nb * 32, (int)(ne - nb), 4, out);
}

// ---- what art_api.cpp calls ---------------------------------------------------------------------------------------------------------
void release_updates(Ctx& c) {
  Ctx::RefitPlan& R = c.refit;
  R.b_idx.release(); R.b_levels.release(); R.b_tight.release(); R.b_bad.release();
  R.level_off.clear(); R.ready = false; R.bad_total = 0; release_lane(R.lane);
  Ctx::MovePlan& P = c.move;
  P.b_plan.release(); P.b_work.release(); P.b_tlas.release(); P.b_blas.release(); P.n_tlas = 0;
  P.level_off.clear(); P.levels = nullptr; P.args = MoveArgs(); P.ready = false; release_lane(P.lane);
  P.meshes.clear(); P.blas_level_off.clear(); P.blas_levels = nullptr; release_lane(P.refit_lane);
}

void destroy_updates(Ctx& c) { release_updates(c); destroy_lane(c.refit.lane); destroy_lane(c.move.lane); destroy_lane(c.move.refit_lane); }

int sync_updates() {
  Ctx& c = g_ctx;
  if (fold_refit()) return 1;
  if (report_bad(c.refit.lane, "art_refit_device: ", " vertex coordinate(s) not finite or beyond 1e18 in magnitude; the boxes "
                 "holding them are empty (no ray enters them) until a good refit or art_upload_scene")) return 1;
  if (fold_move()) return 1;
  if (report_bad(c.move.lane, "art_move_instances_device: ", " instance matrix(es) with an element that is not finite, without an inverse, or "
                 "reaching beyond 1e18; their instances are empty (no ray enters them) until a good move or art_upload_scene")) return 1;
  if (fold_mesh_refit()) return 1;
  return report_bad(c.move.refit_lane, "art_refit_mesh_device: ", " vertex coordinate(s) not finite or beyond 1e18 in magnitude; the boxes and the entry "
                    "points holding them are empty (no ray enters them) until a good refit of their mesh or art_upload_scene");
}

}  // namespace art
