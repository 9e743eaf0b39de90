// art_kernels.h -- launch interface between the host driver (art_api.cpp, art_render.cpp, art_device_entries.cpp) and art_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "art_shade.h"
#include "art_qnode.h"
#include "art_instanced.h"
#include "art_denoise.h"
#include "art_temporal.h"
#include "art_motion.h"
#include "art_adaptive.h"
#include "art_svgf_spatial.h"

namespace art {

enum { TRACE_COOP = 0, TRACE_SIMPLE = 1 };

struct TraceArgs {
  int32_t n_rays;
  int32_t stack_entries;        // per-ray LDS stack depth; >= Bvh8::max_stack unless stack_overflow
  int32_t width;                // node width = lanes per ray in k_trace_coop (8 or 4)
  int32_t instanced;            // DevScene::n_inst > 0: 1 = k_trace_coop<.., INST> walks the two-level tree (qnodes = art_instanced_build.cpp's array), 2 = k_trace_inst (one ray per lane; option inst_coop = 0)
  int32_t stack_overflow;       // the LDS stack is smaller than the tree's bound: pushes are checked, rays that do not fit go to ovf_queue
  int32_t segments;             // k_trace_coop: the queue is cut into this many contiguous segments (1, 2, 4, 8); workgroup b starts
                                // in segment b % segments (its XCD) and moves on to the next segment when that one is drained
  int32_t node_min;             // a wave keeps expanding nodes while at least this many of its 8 ray groups have one
  int32_t refill_min;           // k_trace_coop: idle groups take new rays only when at least this many of the wave's groups are idle (or nothing else is left to do)
  const float* ray_ox; const float* ray_oy; const float* ray_oz;
  const float* ray_dx; const float* ray_dy; const float* ray_dz;
  const float* ray_tfar;        // < 0: skip
  float4* rec;                  // k_analytic -> k_trace_coop: one 64-byte record per QUEUED ray, in queue order (layout below); n_rays + 4096 records (slack for the chunk prefetch)
  // shadow rays (index >= shadow_begin) only feed Compute_Shadow's test  10*eps < t_closest < tfar  (ray_tracer.adb:122):
  // sh_min[i - shadow_begin] = 10*eps.  nullptr: every ray is a closest-hit query.
  const float* sh_min; int32_t shadow_begin;
  DevHit* hit;
  const DevInstance* inst; int32_t inst_shift;   // instanced scene (k_trace_coop<.., INST>): the instance table; a hit's key index = instance << inst_shift | triangle
  float* sh_t;                  // record schedule: a record whose hit-slot word has kShadowWord set leaves its result as ONE float, sh_t[word & ~kShadowWord] = t of the hit (DevPaths::sh_t)
  const float* nodes; const uint32_t* qnodes; const float* tris; const float* qtris; int32_t n_tris;   // qnodes: 64-byte quantised nodes (width 4, art_qnode.h)   // BVH of the closest-hit mesh (hot-loop operands)
  int32_t chunk;                // trace records a wave claims per atomic on the cursor (a multiple of 16: prefetched 16 records per load)
  int* cursor;                  // work cursors, zeroed before every launch: segment k's cursor is cursor[32 * (k + 1)] (cursor[0] serves the
                                // kernels with a single cursor)
  int* queue; int* queue_count; // queue_count: number of trace records k_analytic queued, zeroed before every launch (queue: the same buffer as rec)
  // round 3: the wavefront stages write the records themselves, in item order (DevPaths::rec).  Then the queue length is
  // queue_fixed (>= 0: known on the host), or *queue_items x queue_mul (the output item count of the stage, 1 or 2 records per item)
  int32_t queue_fixed; const int* queue_items; int32_t queue_mul;
  int* ovf_queue; int* ovf_count;   // stack_overflow: rays handed to k_trace_overflow, count zeroed before every launch
  unsigned long long* stats;    // [box, tri, node, leaf, rays] when counting
  unsigned long long* live_rays;   // += closest-hit queries actually issued by this launch (Mrays/s numerator)
  const int* item_count;           // compacted work set: items [0, *item_count) exist (rays [0, n) and [shadow_begin, shadow_begin + n)); nullptr: all n_rays
};

// trace record (4 x float4) of a queued ray: everything k_trace_coop needs to start it, prepared at one ray per lane by k_analytic
//   [0] origin.xyz, starting bound t      [1] direction.xyz, starting bound key      [2] 1/direction (slab_setup), shadow-rule minimum (< 0: closest hit)
//   [3] near-plane byte selector (width 4), ray index, far_found, 0
constexpr int kTraceRecBytes = 64;

void launch_raygen(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q);
void launch_bump(hipStream_t st, unsigned long long* a, unsigned long long* b, unsigned long long n);    // *a += n; if (b) *b += n
// end of a batch: items[b] += input items of bounce b, items[16 + b] += the items it kept (live[32 (b + 1)]); bounce 0 reads the P camera paths
void launch_acc_items(hipStream_t st, const int* live, int depth, int P, unsigned long long* items);
void launch_shade(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q, int bounce);
void launch_finish(hipStream_t st, const DevFrame& F, const DevPaths& Q, int last_level);
// compacted work sets (k_shade_compact): shade the items of Qi, write the survivors densely to Qo (+ their slot ids); n_in nullptr: all Qi.P items
// rays_a / rays_b: += the rays the stage emits as trace records (Qo.rec != nullptr); rays_b may be nullptr
void launch_shade_compact(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Qi, const DevPaths& Qo, int bounce,
                          const int* n_in, int* n_out, uint32_t* slot_out, unsigned long long* lost, unsigned long long* rays_a, unsigned long long* rays_b,
                          int per = 0, int camera_order = 0);      // per: items per thread, 2 or 0 = the default (4); camera_order: bounce 0 visits the slots tile-major (art_camera_order.h)
void launch_resolve_last(hipStream_t st, const DevPaths& Q, const int* n, int last_level);
void launch_fold(hipStream_t st, const DevFrame& F, const DevPaths& Q);
void launch_fold_levels(hipStream_t st, const DevFrame& F, const DevPaths& Q, int max_depth, const int* counts);     // dense fold records: counts[32 k] = items of level k
void launch_accumulate(hipStream_t st, const DevFrame& F, const DevPaths& Q, int samples_in_batch, float* accum);
void launch_accumulate_moments(hipStream_t st, const DevFrame& F, const DevPaths& Q, int samples_in_batch, float* accum, float* moments);   // art_bind_moments: the accum and {S1, S2} in one walk
void launch_resolve(hipStream_t st, const float* accum, int n_pixels, float norm_c, uint32_t* screen);
void launch_debug(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q, float* accum, int32_t* prim_index, int32_t* mat_id, int32_t* prim_type);
void launch_to_xmajor_f3(hipStream_t st, const float* src, float* dst, int w, int h);
void launch_to_xmajor_u32(hipStream_t st, const uint32_t* src, uint32_t* dst, int w, int h);
void launch_from_xmajor_f3(hipStream_t st, const float* src, float* dst, int w, int h);
void launch_trace_instanced(hipStream_t st, const InstScene& T, const float* o, const float* d, const float* tfar, int n, InstHit* out);
void launch_pad_tris(hipStream_t st, const float* src12, float* dst16, int n);
void launch_add_f32(hipStream_t st, const float* src, float* dst, size_t n);
size_t trace_coop_lds_bytes(int stack_entries, int width);
void launch_trace(hipStream_t st, const DevScene* d_scene, const TraceArgs& A, int kernel, bool stats, int grid_blocks);
void launch_analytic(hipStream_t st, const DevScene& scene, const TraceArgs& A, bool stats);
int  trace_coop_blocks_per_cu(int stack_entries, int width);

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
// art_render_aovs_motion_device: the same slice with the motion plane (3 floats per pixel, advanced to the slice; never nullptr here) and
// what its deltas are made from (art_motion.h).  A type of its own, so that the kernels without the plane keep their arguments.
struct AovMotionArgs : AovArgs {
  float* motion;
  mo::Source src;
};
void launch_aov_resolve_motion(hipStream_t st, const DevFrame& F, const DevScene& S, const AovMotionArgs& A);

// art_denoise_device, art_denoise_svgf_device and art_denoise_svgf_var_device (art_denoise.hip, art_device_entries.cpp run_denoise): the caller's planes
// (albedo / normal / depth / variance_out nullptr: not given; out may be color) and the library's scratch records of art_denoise.h, n = W * H
// of each.  moments: the moments plane or, for dn::Mode::SvgfVar, the variance plane (n_colours is then not read).  dn::Mode::Plain leaves
// n_colours, moments, variance_out and z zero: its kernels read none of them.
struct DenoiseArgs {
  dn::Params P;
  int32_t n, n_colours;
  const float* color; const float* moments; const float* albedo; const float* normal; const float* depth;
  float* out; float* variance_out;
  dn::Rec4* image[2]; dn::Rec4* guide; float* z; dn::Rec2* grad;
};
void launch_denoise(hipStream_t st, dn::Mode mode, const DenoiseArgs& A, int iterations);      // the mode's pack kernel and `iterations` filter launches

// art_temporal_device (art_temporal.hip, art_device_entries.cpp temporal_device): the caller's current planes (normal / depth / id nullptr: not given),
// the two histories (hist_in nullptr: the first frame) and the optional outputs; n = W * H of the current frame
struct TemporalArgs {
  tp::Params P;
  int32_t n;
  int32_t has_motion;              // art_temporal_motion_device with a motion plane: the MOTION instantiation runs (the word lies in what was padding)
  const float* color; const float* moments; const float* normal; const float* depth; const int32_t* id;
  const tp::Rec4* hist_in; tp::Rec4* hist_out;
  float* out; float* variance_out; float* length_out;
  const float* motion;             // art_temporal_motion_device: 3 floats per pixel of the current frame; else nullptr
};
void launch_temporal(hipStream_t st, const TemporalArgs& A);      // A.has_motion selects the motion variant of the kernel

// art_compact_mask_device and the masked render pass (art_select.hip): the n entries of a pixel list, the frame's byte mask, one word per
// workgroup of 256 entries (select_blocks(n) words of scratch: counts, then their exclusive prefix sums) and the compacted list
struct SelectArgs {
  const uint8_t* mask; const uint32_t* pixmap; int32_t n;
  uint32_t* block_sums; uint32_t* out;
};
int select_blocks(int n);
void launch_compact_mask(hipStream_t st, const SelectArgs& A, uint32_t* count_out);      // three launches: count, scan (one workgroup), scatter
void launch_add_counts(hipStream_t st, const uint32_t* list, int n, uint32_t* counts, uint32_t samples);   // counts[list[i]] += samples, i < n

// art_adaptive_estimate_device (art_adaptive.hip, art_device_entries.cpp adaptive_estimate_device): the caller's planes, outputs nullptr where not wanted
struct AdaptiveArgs {
  ad::Params P;
  const float* accum; const float* moments; const uint32_t* counts;
  float* mean; float* variance; float* error; uint8_t* mask;
};
void launch_adaptive_estimate(hipStream_t st, const AdaptiveArgs& A);

// art_svgf_spatial_variance_device (art_svgf_spatial.hip, art_device_entries.cpp svgf_spatial_variance_device): the history of art_temporal_device and
// the caller's two variance planes (they may be one); tiles_x = svgf_spatial_tiles_x(P.W), the kernel's tiles per row of tiles
struct SvgfSpatialArgs {
  sv::Params P;
  int32_t tiles_x;
  const sv::Rec4* hist; const float* variance_in; float* variance_out;
};
int svgf_spatial_tiles_x(int width);
void launch_svgf_spatial(hipStream_t st, const SvgfSpatialArgs& A);

// refit of the CLOSEST mesh's tree in place (art_refit.hip, art_update.cpp art_refit_device)
constexpr float kRefitMaxCoord = 1.0e18f;      // the GPU SAH builder's limit: a vertex coordinate beyond it (or not finite) is a bad vertex
struct RefitArgs {
  const float* pos3f; const float* nrm3f;      // the caller's new vertex data (nrm3f nullptr: keep the normals)
  const int32_t* idx;                          // index triples of the mesh (3 per primitive)
  int64_t nverts; int32_t n_prims, n_recs;     // vertices, primitives, triangle records (n_recs > n_prims after spatial splits)
  float* tris; float* qtris; float* m_shade;   // triangle records, their 64-byte padded copy (nullptr at width 8), shading records
  unsigned long long* bad;                     // [0] bad vertices of this refit, [1] cumulative since the upload
  float* nodes; QNode* qnodes;                 // the tree (qnodes nullptr: binary32 boxes only, width 8)
  float* tight;                                // 6 floats per node: the tight box of everything below the node
  int32_t width; float inflate_rel, inflate_abs;
};
void launch_refit_tris(hipStream_t st, const RefitArgs& R);
// art_set_camera (art_refit.hip): the 19 camera words of the scene header in HBM, passed by value so that the host's copy may change at once
struct CameraWords { float w[19]; };           // cam_pos[3], cam_matrix[16]
void launch_set_camera(hipStream_t st, DevScene* d_scene, const CameraWords& C);
void launch_refit_level(hipStream_t st, const RefitArgs& R, const int32_t* level_nodes, int n);

// a new tree from moved vertices and the cost figure of the tree in HBM (art_rebuild.hip, art_update.cpp art_rebuild_device / art_get_tree_cost)
struct GatherArgs {
  const float* pos3f; const int32_t* idx;      // the caller's vertex positions, the mesh's index triples
  int64_t nverts; int32_t n_prims;
  float* tri9;                                 // 9 floats per primitive: what build_bvh8_gpu reads
  unsigned long long* bad;                     // bad vertices of this gather (zeroed by the caller)
};
void launch_gather_tri9(hipStream_t st, const GatherArgs& G);
// sums4 (zeroed by the caller): half areas of the inner child slots | of the leaf slots | of the leaf slots x triangle count | of the root's union
void launch_tree_cost(hipStream_t st, const float* nodes, int n_nodes, int width, double* sums4);

// an instanced scene changes in HBM (art_move.hip): its instances take new matrices (art_update.cpp art_move_instances_device), or one
// of its meshes new vertices (art_refit_mesh_device).  Everything but m12f is the library's: the scene's arrays in HBM and the plan
// (art_instanced_build.h MovePlanHost) next to them.  Both calls end in the same pipeline (launch_move_matrices .. launch_move_tlas_level).
struct MoveArgs {
  const float* m12f;                           // the matrices the pipeline runs at, 12 floats per instance: a move's are the caller's, a mesh refit's are m_cur
  int32_t n_inst, n_entry, n_mesh, n_blas_nodes;
  float* m_cur_out;                            // where the pipeline keeps m12f: a move's m_cur; nullptr for a mesh refit, whose m12f IS m_cur (no kernel reads the array it is writing)
  unsigned long long* bad_total;               // a move counts its bad matrices since the upload here (state + 2); nullptr for a mesh refit, which brings no matrices
  unsigned long long* repads;                  // the meshes this update re-pads are counted here: state + 3 for a move, state + 6 for a mesh refit
  DevInstance* inst;                           // the instance table, one record per entry point
  float* tlas_nodes; float* tlas_tris;         // the instance tree and its proxy records
  float* blas_nodes; const float* blas_tris;   // the meshes' trees and their object-space records (a mesh refit rewrites a mesh's slice before the pipeline runs)
  QNode* qnodes;                               // the merged quantised array: the instance tree first, then every mesh's tree
  const int32_t* range_off; const int32_t* ranges; const int32_t* proxy_rec; const int32_t* inst_mesh;
  const int32_t* mesh_base; const int32_t* node_mesh;
  // state the kernels maintain (the host's copies in TwoLevelHost are stale from the first mesh refit on)
  float* mesh_box;                             // 6 per mesh: the object-space box of its good records
  float* blas_tight;                           // 6 per node of blas_nodes: the tight box of the good records below it (lo > hi: none)
  float* m_cur;                                // 12 per instance: the matrices in force (the uploaded ones, or the last accepted move's)
  float* tlas_tight;                           // 6 floats per node of the instance tree: the tight box below it
  float* ent_box;                              // 6 floats per entry point: its world box (lo > hi: empty -- a bad matrix, or a bad vertex among its records)
  int32_t* inst_ok;                            // per instance: 1 = a good matrix
  unsigned long long* state;                   // [0] the bits of E (binary64, >= 0), [1] bad matrices of this move, [2] since the upload, [3] meshes re-padded by moves since the upload,
                                               // [4] bad vertices of this mesh refit, [5] since the upload, [6] meshes re-padded by mesh refits since the upload,
                                               // [7] bad vertices the meshes hold now (the sum of mesh_bad)
  unsigned long long* mesh_bad;                // per mesh: the bad vertices its last refit left among its records (0: none, or never refitted)
  unsigned long long* needed;                  // per mesh: the bits of the pad this placement asks for (binary64, >= 0)
  float* pad_cur; int32_t* repad;              // per mesh: the pad its boxes carry; 1 = this update widens them
  double extent;                               // the scene's extent without the instances (TwoLevelHost::scene_extent)
  float mesh_pad_rel, mesh_pad_min;            // the meshes' relative pad and the floor of their absolute pad
  float tlas_pad_rel, tlas_pad_abs;            // the instance tree builder's pad rule
};
constexpr int kMoveStateWords = 8;
constexpr double kMoveMaxReach = 1.0e18;       // an instance reaching further out than this (kRefitMaxCoord) has a bad matrix
void launch_move_matrices(hipStream_t st, const MoveArgs& M);                  // begin + matrices + pads
void launch_move_repad(hipStream_t st, const MoveArgs& M);
void launch_move_entry_boxes(hipStream_t st, const MoveArgs& M, bool small);   // small: few records per entry point, one wave each
void launch_move_tlas_level(hipStream_t st, const MoveArgs& M, const int32_t* level_nodes, int n);
// a mesh refit, after launch_refit_tris on the mesh's slices: one level of that mesh's tree (nodes of blas_nodes), then its object-space box
void launch_refit_mesh_level(hipStream_t st, const MoveArgs& M, const int32_t* level_nodes, int n);
void launch_refit_mesh_box(hipStream_t st, const MoveArgs& M, int mesh);

// a new instance tree from the proxy records in HBM (art_move.hip, art_update.cpp art_rebuild_instance_tree_device).  Nothing of the
// scene is written: every kernel reads the scene's arrays and the builder's output and writes buffers the call allocated.
struct InstRebuildArgs {
  int32_t n_entry, n_blas_nodes;
  int32_t n_tlas_old, n_tlas_new;              // nodes of the instance tree in force | of the new one
  const int32_t* order;                        // the upload's proxy order: proxy i is entry point order[i]
  // gather
  const int32_t* proxy_rec; const float* tlas_tris;   // the plan's entry point -> proxy record, the proxy records in force
  float* tri9;                                 // 9 floats per proxy, in the upload's order: what build_bvh_sah_gpu reads
  unsigned long long* bad;                     // [0] proxies without a finite box, [1] leaves of the built tree the finish refused (both zeroed by the caller)
  // finish: the builder's tree (breadth-first numbering, word 9 of a record = the input index) -> the host builder's numbering
  const float* g_nodes; const float* g_tris; const QNode* g_qnodes;
  const int32_t* node_map; const int32_t* rec_map;    // builder's node -> its number in the host builder's order | the same for the records
  float* nodes_out; float* tris_out;           // the new instance tree's packets and proxy records (word 9 = the entry point)
  // relocate
  const QNode* qnodes_old; QNode* qnodes_out;  // the merged array in force | the new one: the finish writes its first n_tlas_new nodes, the relocation the meshes'
  const DevInstance* inst_old; DevInstance* inst_out;
};
void launch_inst_gather(hipStream_t st, const InstRebuildArgs& R);
void launch_inst_finish(hipStream_t st, const InstRebuildArgs& R);
void launch_inst_relocate(hipStream_t st, const InstRebuildArgs& R);

// a new tree for one mesh of an instanced scene from its triangle records in HBM (art_move.hip, art_update.cpp
// art_rebuild_mesh_tree_device).  Nothing of the scene is written: every kernel reads the scene's arrays and the builder's output and
// writes buffers the call allocated.  A tree of another node count moves every mesh behind it by `delta` nodes.
struct MeshRebuildArgs {
  int32_t mesh, n_recs;                        // the mesh; its triangle records (one per triangle)
  int32_t nb, tb, qb;                          // mesh_base of the mesh: first node in blas_nodes, first record in blas_tris, first node in qnodes
  int32_t n_old, n_new, delta;                 // nodes of the mesh's tree in force | of the new one | n_new - n_old
  int32_t n_tlas, n_blas_old, n_entry;         // nodes of the instance tree | of all the meshes' trees in force | entry points
  // gather
  const float* tris_old;                       // blas_tris in force
  float* tri9;                                 // 9 floats per triangle, by its index in the mesh (word 9 of a record): what build_bvh_sah_gpu reads
  unsigned long long* bad;                     // [0] records whose index is out of range or whose corners are not finite, [1] leaves of the built tree the finish refused (both zeroed by the caller)
  // finish: the builder's tree (breadth-first numbering, mesh-relative entry words) -> the host builder's numbering inside the new arrays
  const float* g_nodes; const float* g_tris; const QNode* g_qnodes;
  const int32_t* node_map; const int32_t* rec_map;    // builder's node -> its number in the host builder's order | the same for the records
  float* nodes_out; float* tris_out; float* qtris_out; QNode* qnodes_out;   // the new blas_nodes, blas_tris, padded copy and merged quantised array
  int32_t* node_mesh_out; float* tight_out;    // the plan's per-node arrays over the new blas_nodes
  // relocate
  const float* nodes_old; const QNode* qnodes_old; const int32_t* node_mesh_old; const float* tight_old;
  const DevInstance* inst_old; DevInstance* inst_out; const int32_t* inst_mesh;
};
void launch_mesh_gather(hipStream_t st, const MeshRebuildArgs& R);
void launch_mesh_finish(hipStream_t st, const MeshRebuildArgs& R);
void launch_mesh_relocate(hipStream_t st, const MeshRebuildArgs& R);
void launch_mesh_tight_level(hipStream_t st, const MeshRebuildArgs& R, const int32_t* level_nodes, int n);   // after the finish, deepest level first: nodes of the new blas_nodes

}  // namespace art
