// art_move.h -- launch interface of art_move.hip: the updates of an instanced scene in HBM (instances moved, a mesh refitted) and
// the rebuilds of its instance tree and of one mesh's tree.
#pragma once
#include <hip/hip_runtime.h>
#include "art_scene.h"

namespace art {

struct QNode;      // art_qnode.h

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
