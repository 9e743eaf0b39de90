// art_refit.h -- launch interface of art_refit.hip: the refit of the closest-hit mesh's tree in place, and the camera words.
#pragma once
#include <hip/hip_runtime.h>
#include "art_scene.h"

namespace art {

struct QNode;      // art_qnode.h

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

}  // namespace art
