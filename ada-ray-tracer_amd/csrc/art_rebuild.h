// art_rebuild.h -- launch interface of art_rebuild.hip: the builder's input from moved vertices, and the cost figure of a tree in HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace art {

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

}  // namespace art
