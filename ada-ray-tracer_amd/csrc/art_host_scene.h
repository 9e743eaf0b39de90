// art_host_scene.h -- validation + flattening of an ArtSceneDesc into the packed host arrays that are
// copied to HBM (and, in the host-simulation test build, consumed directly).  Scene.Init's job.
#pragma once
#include <string>
#include <vector>
#include "../../include/art_hip.h"
#include "art_bvh.h"
#include "art_scene.h"
#include "art_instanced_build.h"

namespace art {

struct HostScene {
  float extent_rest = 0.0f;           // instanced scenes: the scene extent without the camera (walls, spheres, lights); art_set_camera adds the camera's reach again
  std::vector<DevSphere> spheres; std::vector<int32_t> sphere_mat;
  std::vector<DevLight> lights;
  std::vector<DevMaterial> materials;
  // brute-force (reference) mesh
  std::vector<float> bf_pos, bf_nrm, bf_uv; std::vector<int32_t> bf_idx;
  int32_t bf_ntris = 0;
  // closest-hit mesh
  std::vector<float> m_shade;   // kTriShadeFloats per triangle: vertex normals of A, B, C and the material id (art_scene.h)
  std::vector<float> m_pos;   // the uploaded vertex positions (nothing in the library reads them back; art_refit_device empties them: they would be stale)
  std::vector<int32_t> m_idx; int64_t m_nverts = 0;   // index triples and vertex count of the CLOSEST mesh: what art_refit_device gathers through (copied to HBM on the first refit)
  Bvh8 bvh;
  std::vector<float> deferred_tri9;   // builder == 1: triangle corners for the GPU build (bvh stays empty until then)
  bool gpu_built = false;             // nodes / tris live only in HBM (art_export_bvh copies them back on demand)
  bool refitted = false;              // art_refit_device moved the tree's boxes: the HBM copy is the only current one, whichever builder made it
  bool m_shade_stale = false;         // art_refit_device rewrote the normals in HBM: art_trace_rays copies m_shade back before it reads it
  bool inst_stale = false;            // art_move_instances_device rewrote the instance table in HBM: art_trace_rays copies `inst` back before it reads it
  bool gcore_seam = false;           // committed by gcore_commit_scene (which keeps its own host copy of the tree: not refittable)
  bool tree_in_hbm_only() const { return gpu_built || refitted; }
  double bvh_build_ms = 0.0;
  // instanced scene (ArtSceneDesc::n_instances > 0): m_shade then holds the MESHES' records (object-space normals), one block per mesh
  // (`two` is the build as uploaded: art_refit_mesh_device leaves its records and boxes stale, and nothing reads them after the update plan is built)
  TwoLevelHost two; std::vector<DevInstance> inst;
  // what art_refit_mesh_device gathers through, per mesh of ArtSceneDesc::meshes: the vertex count, and the index triples of every mesh an
  // instance shows, mesh m's at mesh_idx[mesh_idx_off[m] .. mesh_idx_off[m + 1]) (copied to HBM with the update plan)
  std::vector<int32_t> mesh_idx; std::vector<int64_t> mesh_idx_off; std::vector<int32_t> mesh_nverts;
  DevScene hdr;               // scalar part; pointer members are filled by the owner (host or device addresses)
};

// the explicit flattening of an instanced scene's meshes -- what an instanced render must equal bit for bit: positions, normals (3 floats per
// vertex), indices, material ids of ONE world-space mesh, triangles in the order (instance, triangle of the mesh)
bool flatten_instances(const ArtSceneDesc& d, std::vector<float>& pos, std::vector<float>& nrm, std::vector<int32_t>& idx, std::vector<int32_t>& matid, std::string& err);


bool flatten_scene(const ArtSceneDesc& d, const BvhBuildParams& bp, HostScene& out, std::string& err);

// pixel ownership for multi-GPU sharding: tile x tile pixel tiles dealt along diagonals, (bx + s by) % nranks == rank (s = 3, or 5 / 7 when 3 divides nranks).
// Returns the global pixel indices (y*W + x) owned by `rank`, in tile order.
std::vector<uint32_t> build_pixmap(int W, int H, int rank, int nranks, int tile);

// points hdr's pointer members at the host vectors (host simulation / CPU-side checks)
void bind_host_pointers(HostScene& hs);

}  // namespace art
