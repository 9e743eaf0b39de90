// art_move.hip -- gfx950 kernels of the device-side updates of an instanced scene.  art_move_instances_device: the instances take new
// object -> world matrices.  Topology, entry points and the meshes' records stay as built; matrices and boxes are rewritten, in this
// order (one launch each, every launch reads only what earlier launches wrote: gfx950's per-XCD L2s are not coherent within a launch):
//
//   k_move_begin        E = the scene's extent without the instances, this move's bad count = 0, every mesh's needed pad = 0.
//   k_move_matrices     one lane per entry-point record: DevInstance::m, and minv in invert_3x4's arithmetic (art_instanced_build.cpp:
//                       binary64, rounded once -- the bytes an upload writes).  The first n_inst lanes (one per instance) count the bad
//                       matrices, raise E to the instance's reach (atomicMax on the bits of a non-negative binary64) and, for a move,
//                       keep the matrix in m_cur (m_cur_out).  The matrices are read from m12f -- the caller's for a move, m_cur for a mesh
//                       refit, which passes no m_cur_out: the kernel never reads the array it is writing.
//   k_move_pads_inst    one lane per instance: the upload's bound 8 * 2^-24 * (sum_j |minv_rj| * 3 E + |minv_r3|), maximised over the rows,
//                       folded into needed[mesh].
//   k_move_pads_mesh    one lane per mesh: repad = needed > current, current = max(current, needed).  Pads only grow.
//   k_move_repad        one lane per node of the meshes' trees; a lane whose mesh is not re-padded returns at once.  The others run
//                       refit_node (art_refit_node.h: the rules of a node refit are stated there) with inflate_abs = current[mesh].  The
//                       tight box below every node is state of the plan that earlier launches left (blas_tight), so the whole forest
//                       is one launch, not one per level, and no tight union is written.  The entry words of the merged quantised array
//                       are absolute and stay as stored: only planes and header are rewritten.
//   k_move_entry_boxes  one workgroup per entry point: the three corners of every record below it through world_box's arithmetic
//                       (binary64 products and sums, the four-term pad, one rounding) -- the upload's tight box -- and its proxy record.
//                       A record with a bad coordinate (a bad mesh refit left it) never reaches that arithmetic: its entry point gets
//                       the empty box.
//   k_move_tlas_level   one launch per level of the instance tree, deepest first: refit_node with a leaf child's box taken from its
//                       proxies' entry points under the builder's pad rule, an inner child's from the tight box below; instance markers kept.
//
// A bad matrix (an element not finite, a determinant failing invert_3x4's test, or a reach beyond kMoveMaxReach) gives every entry
// point of its instance an empty box, which refit_node treats as it treats a box with a bad vertex.
//
// art_refit_mesh_device: one mesh takes new vertices.  k_refit_tris (art_refit.hip) rewrites the mesh's slices of the records, then
//
//   k_refit_mesh_level  one launch per level of THAT mesh's tree, deepest first, one lane per node: refit_node with inflate_abs =
//                       current[mesh], a leaf child's box from its records, an inner child's from blas_tight; the node's tight union
//                       goes to blas_tight.  (k_move_repad is the same node refit without the tight union.)
//   k_refit_mesh_box    mesh_box[mesh] = the tight box stored for the mesh's root; an empty one (every record bad) keeps the previous box.
//                       mesh_bad[mesh] = the bad vertices k_refit_tris counted, and their sum over the meshes: what art_synchronize reports
//                       is what the meshes hold now, so a good refit of ANOTHER mesh does not hide a mesh that is still bad.
//
// and the pipeline above runs at the matrices in force: E depends on mesh_box and every mesh's pad on E, so a mesh that grows can widen
// another mesh's pad, and every entry point's box depends on the records below it.
//
// art_rebuild_instance_tree_device: the instance tree is built again from the proxy records in HBM.  The GPU binned-SAH builder
// (art_sah.hip) does the building; around it
//
//   k_inst_gather       one lane per proxy in the upload's order: the entry point's box (corners 0 and 1 of its proxy record: the upload's
//                       tight box, which a move or a mesh refit keeps up to date) as the 9-float triangle the upload feeds its builder.
//                       A box that is not finite, inverted or beyond kRefitMaxCoord is counted; the host reads the count before the
//                       builder starts.
//   k_inst_finish       one lane per node of the built tree.  The builder numbers nodes breadth-first and records by reference position,
//                       the host builder depth-first (art_bvh.cpp's collapse); the host has read the built tree's reference words back and
//                       hands over both renumberings.  The lane writes its node's packet and quantised form at the host builder's number
//                       with the references renumbered, every leaf's record at its new place with word 9 = the entry point (the builder
//                       left the input index there), and the leaf's entry word as an instance marker.  A leaf that does not hold exactly
//                       one record inside the array is counted and left empty (the host has refused that tree already: nothing is committed).
//   k_inst_relocate     the meshes' quantised nodes behind the new instance tree: inner entry words move by the change in the instance
//                       tree's node count, leaf words stay; and a copy of the instance table with every non-leaf qroot moved likewise.
//
// art_rebuild_mesh_tree_device: one mesh's tree is built again from its triangle records in HBM, by the same builder; around it
//
//   k_mesh_gather       one lane per record of the mesh: its corners go to tri9 at the triangle's index in the mesh (word 9), the order an
//                       upload feeds them in.  An index out of range or a corner that is not finite or beyond kRefitMaxCoord is counted;
//                       the host reads the count before the builder starts.
//   k_mesh_finish       one lane per 16-byte lane record: lane j of a node's four takes child slot j -- the packet's two rows and the
//                       quantised record -- to the host builder's number inside the mesh's new slices, references renumbered, entry
//                       words made absolute; lane q of a triangle record's four writes quarter q of the record at its new place and of
//                       its 64-byte padded copy (quarter 3: the padding).  A leaf outside the records is counted and left empty (the host
//                       has refused that tree already).
//   k_mesh_relocate     one lane per 16 bytes of what the other meshes keep: their packets, their quantised nodes (and the instance
//                       tree's), the instance table, and per node the plan's node_mesh and blas_tight.  A mesh behind the rebuilt one moves
//                       by the change in its node count: its inner entry words, its instances' node_base and every qroot that names a node.
//   k_mesh_tight_level  one launch per level of the new tree, deepest first: the tight box below every node, for the plan's blas_tight.
//
// None of these writes anything the scene in force reads: the driver swaps the new buffers in once every context has built.
#include <hip/hip_runtime.h>

#include "art_bvh.h"
#include "art_move.h"
#include "art_refit_node.h"

namespace art {

constexpr int kMoveBlock = 128;

__device__ __forceinline__ bool move_invert_3x4(const float m[12], float out[12]) {      // art_instanced_build.cpp invert_3x4, expression for expression
  const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g0 = m[8], h = m[9], i = m[10];
  const double det = a * (e * i - f * h) - b * (d * i - f * g0) + c * (d * h - e * g0);
  if (!(fabs(det) > 1.0e-300) || !isfinite(det)) return false;
  const double r[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                       (f * g0 - d * i) / det, (a * i - c * g0) / det, (c * d - a * f) / det,
                       (d * h - e * g0) / det, (b * g0 - a * h) / det, (a * e - b * d) / det};
  for (int row = 0; row < 3; ++row) {
    for (int k = 0; k < 3; ++k) out[4 * row + k] = (float)r[3 * row + k];
    out[4 * row + 3] = (float)-(r[3 * row] * (double)m[3] + r[3 * row + 1] * (double)m[7] + r[3 * row + 2] * (double)m[11]);
  }
  return true;
}

__device__ __forceinline__ double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off));
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off));
  return v;
}

__global__ __launch_bounds__(kMoveBlock) void k_move_begin(const MoveArgs M) {
  const int t = blockIdx.x * kMoveBlock + threadIdx.x;
  if (t == 0) { M.state[0] = (unsigned long long)__double_as_longlong(M.extent); M.state[1] = 0ull; }
  if (t < M.n_mesh) M.needed[t] = 0ull;
}

__global__ __launch_bounds__(kMoveBlock) void k_move_matrices(const MoveArgs M) {
  const int e = blockIdx.x * kMoveBlock + threadIdx.x;
  double reach_max = 0.0;
  bool first = false;
  if (e < M.n_entry) {
    DevInstance* const D = M.inst + e;
    const int inst = D->inst;
    float m[12], minv[12];
    bool ok = true;
    for (int k = 0; k < 12; ++k) { m[k] = M.m12f[12 * (size_t)inst + k]; ok = ok && isfinite(m[k]); }
    const bool inv = ok && move_invert_3x4(m, minv);
    ok = inv;
    const float* mb = M.mesh_box + 6 * (size_t)M.inst_mesh[inst];
    for (int r = 0; r < 3; ++r) {                                          // how far out the instance reaches in the world
      double reach = fabs((double)m[4 * r + 3]);
      for (int j = 0; j < 3; ++j) reach += fabs((double)m[4 * r + j]) * fmax(fabs((double)mb[j]), fabs((double)mb[j + 3]));
      if (!(reach <= kMoveMaxReach)) ok = false;                           // (also a NaN)
      else reach_max = fmax(reach_max, reach);
    }
    for (int k = 0; k < 12; ++k) { D->m[k] = m[k]; D->minv[k] = inv ? minv[k] : 0.0f; }
    first = (e < M.n_inst);
    if (first) {                                                           // (record e < n_inst is instance e)
      M.inst_ok[e] = ok ? 1 : 0;
      if (!ok) { atomicAdd(&M.state[1], 1ull); if (M.bad_total) atomicAdd(M.bad_total, 1ull); }
      if (M.m_cur_out) for (int k = 0; k < 12; ++k) M.m_cur_out[12 * (size_t)e + k] = m[k];
    }
    if (!first || !ok) reach_max = 0.0;
  }
  const double wm = wave_max(reach_max);                                   // (every lane of the wave takes part)
  if ((threadIdx.x & 63) == 0 && wm > 0.0) atomicMax(&M.state[0], (unsigned long long)__double_as_longlong(wm));
}

__global__ __launch_bounds__(kMoveBlock) void k_move_pads_inst(const MoveArgs M) {
  const int i = blockIdx.x * kMoveBlock + threadIdx.x;
  if (i >= M.n_inst || !M.inst_ok[i]) return;
  const double E = __longlong_as_double((long long)M.state[0]);
  const float* q0 = M.inst[i].minv;
  double best = 0.0;
  for (int r = 0; r < 3; ++r) {
    const float* q = q0 + 4 * r;
    const double bound = 8.0 * 5.9604644775390625e-8 * ((fabs((double)q[0]) + fabs((double)q[1]) + fabs((double)q[2])) * 3.0 * E + fabs((double)q[3]));
    if (isfinite(bound)) best = fmax(best, bound);
  }
  const unsigned long long bits = (unsigned long long)__double_as_longlong(best);
  unsigned long long* const cell = M.needed + M.inst_mesh[i];
  if (bits > *cell) atomicMax(cell, bits);                                 // (a stale read is a smaller value: the atomic is then issued for nothing, never skipped wrongly)
}

__global__ __launch_bounds__(kMoveBlock) void k_move_pads_mesh(const MoveArgs M) {
  const int m = blockIdx.x * kMoveBlock + threadIdx.x;
  if (m >= M.n_mesh) return;
  const double need = __longlong_as_double((long long)M.needed[m]);
  const float nf = fmaxf(M.mesh_pad_min, (float)fmin(need, 1.0e30));
  const bool rp = nf > M.pad_cur[m];
  M.repad[m] = rp ? 1 : 0;
  if (rp) { M.pad_cur[m] = nf; atomicAdd(M.repads, 1ull); }
}

// node g of blas_nodes, a node of mesh mi's tree, under the pad the mesh carries now; tight_out: where its tight union goes (nullptr: not wanted)
__device__ __forceinline__ void refit_mesh_node(const MoveArgs& M, int g, int mi, float* tight_out) {
  const int32_t nb = M.mesh_base[3 * mi], tb = M.mesh_base[3 * mi + 1], qb = M.mesh_base[3 * mi + 2];
  if (tb < 0) return;                                                      // (a mesh nobody shows)
  const float pad_abs = M.pad_cur[mi];
  refit_node<4, QEntries::kKeep>(M.blas_nodes + (size_t)g * 32, M.qnodes + (size_t)qb + (size_t)(g - nb), tight_out, M.mesh_pad_rel, pad_abs,
                                 [&](int, int32_t ref, int32_t cnt, float l[3], float h[3]) {
    return cnt > 0 ? records_box(M.blas_tris + (size_t)kTriFloats * (size_t)(tb + ref), cnt, l, h) : stored_box(M.blas_tight + 6 * (size_t)(nb + ref), l, h);
  });
}

__global__ __launch_bounds__(kMoveBlock) void k_move_repad(const MoveArgs M) {
  const int g = blockIdx.x * kMoveBlock + threadIdx.x;
  if (g >= M.n_blas_nodes) return;
  const int mi = M.node_mesh[g];
  if (!M.repad[mi]) return;
  refit_mesh_node(M, g, mi, nullptr);
}

__global__ __launch_bounds__(kMoveBlock) void k_refit_mesh_level(const MoveArgs M, const int32_t* __restrict__ level, int n) {
  const int t = blockIdx.x * kMoveBlock + threadIdx.x;
  if (t >= n) return;
  const int g = level[t];
  refit_mesh_node(M, g, M.node_mesh[g], M.blas_tight + 6 * (size_t)g);
}

__global__ void k_refit_mesh_box(const MoveArgs M, int mesh) {
  const float* t = M.blas_tight + 6 * (size_t)M.mesh_base[3 * mesh];       // the mesh's root
  if (threadIdx.x < 6 && t[0] <= t[3]) M.mesh_box[6 * (size_t)mesh + threadIdx.x] = t[threadIdx.x];
  unsigned long long held = 0ull;                                          // this refit's count replaces the mesh's; the other meshes keep theirs
  for (int m = threadIdx.x; m < M.n_mesh; m += 64) held += (m == mesh) ? M.state[4] : M.mesh_bad[m];
  for (int off = 32; off > 0; off >>= 1) held += __shfl_down(held, off);   // (one wave: launch_refit_mesh_box)
  if (threadIdx.x == 0) { M.mesh_bad[mesh] = M.state[4]; M.state[7] = held; }
}

template <int B>
__global__ __launch_bounds__(B) void k_move_entry_boxes(const MoveArgs M) {
  const int e = blockIdx.x, tid = threadIdx.x;
  const DevInstance* const D = M.inst + e;
  float* const box = M.ent_box + 6 * (size_t)e;
  if (!M.inst_ok[D->inst]) {                                               // (the same for the whole workgroup)
    if (tid == 0) { box[0] = box[1] = box[2] = INFINITY; box[3] = box[4] = box[5] = -INFINITY; }
    return;
  }
  double Mx[12];
  for (int k = 0; k < 12; ++k) Mx[k] = (double)D->m[k];
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, mag[3] = {0.0, 0.0, 0.0};
  bool bad = false;
  for (int k = M.range_off[e]; k < M.range_off[e + 1]; ++k) {
    const int32_t first = M.ranges[2 * k], n3 = 3 * M.ranges[2 * k + 1];
    for (int c = tid; c < n3; c += B) {
      const float* p = M.blas_tris + (size_t)kTriFloats * (size_t)(first + c / 3) + 3 * (c % 3);
      if (!(coord_ok(p[0]) && coord_ok(p[1]) && coord_ok(p[2]))) { bad = true; continue; }      // (a bad vertex of a mesh refit: kept out of the arithmetic below)
      const double x = p[0], y = p[1], z = p[2];
      for (int r = 0; r < 3; ++r) {                                        // world_box of art_instanced_build.cpp
        const double a = Mx[4 * r] * x, b = Mx[4 * r + 1] * y, cc = Mx[4 * r + 2] * z, w = a + b + cc + Mx[4 * r + 3];
        lo[r] = fmin(lo[r], w); hi[r] = fmax(hi[r], w);
        mag[r] = fmax(mag[r], fabs(a) + fabs(b) + fabs(cc) + fabs(Mx[4 * r + 3]));
      }
    }
  }
  if (__syncthreads_or(bad ? 1 : 0)) {                                     // (every lane of the workgroup arrives here)
    if (tid == 0) { box[0] = box[1] = box[2] = INFINITY; box[3] = box[4] = box[5] = -INFINITY; }
    return;
  }
  __shared__ double red[(B / 64) * 9];
  for (int r = 0; r < 3; ++r) { lo[r] = wave_min(lo[r]); hi[r] = wave_max(hi[r]); mag[r] = wave_max(mag[r]); }
  if (B > 64) {
    if ((tid & 63) == 0) for (int r = 0; r < 3; ++r) { red[9 * (tid >> 6) + r] = lo[r]; red[9 * (tid >> 6) + 3 + r] = hi[r]; red[9 * (tid >> 6) + 6 + r] = mag[r]; }
    __syncthreads();
  }
  if (tid != 0) return;
  for (int w = 1; w < B / 64; ++w)
    for (int r = 0; r < 3; ++r) { lo[r] = fmin(lo[r], red[9 * w + r]); hi[r] = fmax(hi[r], red[9 * w + 3 + r]); mag[r] = fmax(mag[r], red[9 * w + 6 + r]); }
  float flo[3], fhi[3];
  for (int r = 0; r < 3; ++r) {
    const double pad = 1.0e-4 * (hi[r] - lo[r]) + 1.0e-5 * fmax(fabs(lo[r]), fabs(hi[r])) + 1.0e-6 * mag[r] + 1.0e-6;
    flo[r] = (float)(lo[r] - pad); fhi[r] = (float)(hi[r] + pad);
  }
  for (int r = 0; r < 3; ++r) { box[r] = flo[r]; box[3 + r] = fhi[r]; }
  float* const p = M.tlas_tris + (size_t)kTriFloats * (size_t)M.proxy_rec[e];   // ONE triangle whose corners span the box
  p[0] = flo[0]; p[1] = flo[1]; p[2] = flo[2]; p[3] = fhi[0]; p[4] = fhi[1]; p[5] = fhi[2]; p[6] = flo[0]; p[7] = fhi[1]; p[8] = flo[2];
}

__global__ __launch_bounds__(kMoveBlock) void k_move_tlas_level(const MoveArgs M, const int32_t* __restrict__ level, int n) {
  const int t = blockIdx.x * kMoveBlock + threadIdx.x;
  if (t >= n) return;
  const int node = level[t];
  refit_node<4, QEntries::kKeep>(M.tlas_nodes + (size_t)node * 32, M.qnodes + node, M.tlas_tight + 6 * (size_t)node, M.tlas_pad_rel, M.tlas_pad_abs,
                                 [&](int, int32_t ref, int32_t cnt, float l[3], float h[3]) {
    if (cnt <= 0) return stored_box(M.tlas_tight + 6 * (size_t)ref, l, h);
    l[0] = l[1] = l[2] = INFINITY; h[0] = h[1] = h[2] = -INFINITY;
    for (int r = 0; r < cnt && r < kMaxLeafTris; ++r) {                     // the proxies of the leaf: each names its entry point (an empty box adds nothing)
      const int32_t ent = __float_as_int(M.tlas_tris[(size_t)kTriFloats * (size_t)(ref + r) + 9]);
      const float* b = M.ent_box + 6 * (size_t)ent;
      for (int a = 0; a < 3; ++a) { l[a] = fminf(l[a], b[a]); h[a] = fmaxf(h[a], b[3 + a]); }
    }
    return l[0] <= h[0];                                                    // false: nothing good below
  });
}

// ---- art_rebuild_instance_tree_device ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMoveBlock) void k_inst_gather(const InstRebuildArgs R) {
  const int i = blockIdx.x * kMoveBlock + threadIdx.x;
  if (i >= R.n_entry) return;
  const float* p = R.tlas_tris + (size_t)kTriFloats * (size_t)R.proxy_rec[R.order[i]];      // (the host checked both index arrays)
  const float lo[3] = {p[0], p[1], p[2]}, hi[3] = {p[3], p[4], p[5]};
  bool ok = true;
  for (int a = 0; a < 3; ++a) ok = ok && fabsf(lo[a]) <= kRefitMaxCoord && fabsf(hi[a]) <= kRefitMaxCoord && lo[a] <= hi[a];      // (false for NaN and +-inf)
  if (!ok) atomicAdd(R.bad, 1ull);
  float* t = R.tri9 + 9 * (size_t)i;                                       // ONE triangle whose corners span the box
  t[0] = lo[0]; t[1] = lo[1]; t[2] = lo[2]; t[3] = hi[0]; t[4] = hi[1]; t[5] = hi[2]; t[6] = lo[0]; t[7] = hi[1]; t[8] = lo[2];
}

__global__ __launch_bounds__(kMoveBlock) void k_inst_finish(const InstRebuildArgs R) {
  const int n = blockIdx.x * kMoveBlock + threadIdx.x;
  if (n >= R.n_tlas_new) return;
  const int dst = R.node_map[n];                                           // (a permutation of the nodes: the host built it from the tree it checked)
  const float* src = R.g_nodes + (size_t)n * 32;
  float* out = R.nodes_out + (size_t)dst * 32;
  QNode q = R.g_qnodes[n];
  for (int j = 0; j < 4; ++j) {
    int32_t ref = __float_as_int(src[4 * j + 3]);
    const int32_t cnt = __float_as_int(src[16 + 4 * j + 3]);
    if (ref >= 0 && cnt == 0) {
      ref = (ref < R.n_tlas_new) ? R.node_map[ref] : 0;
      q.rec[j].entry = (uint32_t)ref * (uint32_t)kQNodeBytes;
    } else if (ref >= 0) {
      const int32_t idx = (cnt == 1 && ref < R.n_entry) ? __float_as_int(R.g_tris[(size_t)kTriFloats * (size_t)ref + 9]) : -1;
      if (idx < 0 || idx >= R.n_entry) { atomicAdd(R.bad + 1, 1ull); q.rec[j].entry = kQEntryEmpty; ref = -1; }
      else {
        const int32_t ent = R.order[idx], rec = R.rec_map[ref];
        const float* ts = R.g_tris + (size_t)kTriFloats * (size_t)ref;
        float* td = R.tris_out + (size_t)kTriFloats * (size_t)rec;
        for (int k = 0; k < kTriFloats; ++k) td[k] = ts[k];
        td[9] = __int_as_float(ent);
        q.rec[j].entry = kQEntryLeaf | ((uint32_t)ent << 4) | kQCountInstance;
        ref = rec;
      }
    }
    for (int k = 0; k < 3; ++k) { out[4 * j + k] = src[4 * j + k]; out[16 + 4 * j + k] = src[16 + 4 * j + k]; }
    out[4 * j + 3] = __int_as_float(ref); out[16 + 4 * j + 3] = src[16 + 4 * j + 3];
  }
  R.qnodes_out[dst] = q;
}

__global__ __launch_bounds__(kMoveBlock) void k_inst_relocate(const InstRebuildArgs R) {
  const int t = blockIdx.x * kMoveBlock + threadIdx.x;
  const uint32_t shift = (uint32_t)(R.n_tlas_new - R.n_tlas_old) * (uint32_t)kQNodeBytes;      // (modulo 2^32: a smaller tree moves the words down)
  if (t < R.n_blas_nodes) {
    QNode q = R.qnodes_old[(size_t)R.n_tlas_old + (size_t)t];
    for (int j = 0; j < 4; ++j) if (!(q.rec[j].entry & kQEntryLeaf)) q.rec[j].entry += shift;      // (an empty slot is a leaf of no records)
    R.qnodes_out[(size_t)R.n_tlas_new + (size_t)t] = q;
  }
  if (t < R.n_entry) {
    DevInstance d = R.inst_old[t];
    if (!(d.qroot & kQEntryLeaf)) d.qroot += shift;
    R.inst_out[t] = d;
  }
}

// ---- art_rebuild_mesh_tree_device --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMoveBlock) void k_mesh_gather(const MeshRebuildArgs R) {
  const int i = blockIdx.x * kMoveBlock + threadIdx.x;
  if (i >= R.n_recs) return;
  const float* p = R.tris_old + (size_t)kTriFloats * (size_t)(R.tb + i);
  const int32_t prim = __float_as_int(p[9]);
  bool ok = (uint32_t)prim < (uint32_t)R.n_recs;
  for (int k = 0; k < 9; ++k) ok = ok && coord_ok(p[k]);
  if (!ok) { atomicAdd(R.bad, 1ull); return; }
  float* t = R.tri9 + 9 * (size_t)prim;
  for (int k = 0; k < 9; ++k) t[k] = p[k];
}

__global__ __launch_bounds__(kMoveBlock) void k_mesh_finish(const MeshRebuildArgs R) {
  const int t = blockIdx.x * kMoveBlock + threadIdx.x;
  const int i = t >> 2, j = t & 3;
  if (i < R.n_new) {
    const int dst = R.node_map[i];                                         // (a permutation of the nodes: the host built it from the tree it checked)
    const float4* src = reinterpret_cast<const float4*>(R.g_nodes + (size_t)i * 32);
    float4 lo = src[j], hi = src[4 + j];
    uint4 q = reinterpret_cast<const uint4*>(R.g_qnodes + i)[j];
    int32_t ref = __float_as_int(lo.w);
    const int32_t cnt = __float_as_int(hi.w);
    if (ref >= 0 && cnt == 0) {
      ref = (ref < R.n_new) ? R.node_map[ref] : 0;
      q.z = (uint32_t)(R.qb + ref) * (uint32_t)kQNodeBytes;
    } else if (ref >= 0) {
      if (cnt < 1 || cnt > 4 || ref > R.n_recs - cnt) { atomicAdd(R.bad + 1, 1ull); q.z = kQEntryEmpty; ref = -1; }
      else {
        ref = R.rec_map[ref];                                              // (a leaf's records stay one after the other, in the builder's order)
        q.z = kQEntryLeaf | ((uint32_t)(R.tb + ref) * (uint32_t)kQTriBytes) | (uint32_t)cnt;
      }
    }
    lo.w = __int_as_float(ref);
    float4* out = reinterpret_cast<float4*>(R.nodes_out + (size_t)(R.nb + dst) * 32);
    out[j] = lo; out[4 + j] = hi;
    reinterpret_cast<uint4*>(R.qnodes_out + (size_t)R.qb + (size_t)dst)[j] = q;
    if (j == 0) R.node_mesh_out[R.nb + dst] = R.mesh;
  }
  if (i < R.n_recs) {
    const size_t rec = (size_t)R.tb + (size_t)R.rec_map[i];
    const float4 v = (j < 3) ? reinterpret_cast<const float4*>(R.g_tris + (size_t)kTriFloats * (size_t)i)[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (j < 3) reinterpret_cast<float4*>(R.tris_out + (size_t)kTriFloats * rec)[j] = v;
    reinterpret_cast<float4*>(R.qtris_out + (size_t)(kQTriBytes / 4) * rec)[j] = v;
  }
}

__global__ __launch_bounds__(kMoveBlock) void k_mesh_relocate(const MeshRebuildArgs R) {
  const int64_t t = (int64_t)blockIdx.x * kMoveBlock + threadIdx.x;
  const int32_t first = R.nb, end = R.nb + R.n_old;                        // the rebuilt mesh's nodes in the arrays in force: not copied
  const uint32_t shift = (uint32_t)R.delta * (uint32_t)kQNodeBytes;        // (modulo 2^32: a smaller tree moves the words down)
  if (t < 8 * (int64_t)R.n_blas_old) {                                     // packets: mesh-relative references, copied as they are
    const int64_t g = t >> 3;
    if (g < first || g >= end) reinterpret_cast<uint4*>(R.nodes_out)[(g < first ? g : g + R.delta) * 8 + (t & 7)] = reinterpret_cast<const uint4*>(R.nodes_old)[t];
  }
  if (t < 4 * ((int64_t)R.n_tlas + R.n_blas_old)) {                        // quantised nodes: the instance tree's, then the meshes'
    const int64_t n = t >> 2, g = n - R.n_tlas;
    if (g < first || g >= end) {
      uint4 q = reinterpret_cast<const uint4*>(R.qnodes_old)[t];
      if (g >= end && !(q.z & kQEntryLeaf)) q.z += shift;                  // (an empty slot is a leaf of no records; record positions do not move)
      reinterpret_cast<uint4*>(R.qnodes_out)[(g < first ? n : n + R.delta) * 4 + (t & 3)] = q;
    }
  }
  if (t < 8 * (int64_t)R.n_entry) {                                        // the instance table: lane record 6 holds node_base, 7 qroot and inst
    const int64_t e = t >> 3;
    const int k = (int)(t & 7);
    uint4 v = reinterpret_cast<const uint4*>(R.inst_old)[t];
    if (k >= 6 && R.inst_mesh[R.inst_old[e].inst] > R.mesh) {
      if (k == 6) v.x += (uint32_t)R.delta;
      else if (!(v.x & kQEntryLeaf)) v.x += shift;
    }
    reinterpret_cast<uint4*>(R.inst_out)[t] = v;
  }
  if (t < R.n_blas_old && (t < first || t >= end)) {                       // the plan's per-node arrays
    const int64_t d = t < first ? t : t + R.delta;
    R.node_mesh_out[d] = R.node_mesh_old[t];
    for (int k = 0; k < 6; ++k) R.tight_out[6 * d + k] = R.tight_old[6 * t + k];
  }
}

__global__ __launch_bounds__(kMoveBlock) void k_mesh_tight_level(const MeshRebuildArgs R, const int32_t* __restrict__ level, int n) {
  const int t = blockIdx.x * kMoveBlock + threadIdx.x;
  if (t >= n) return;
  const int g = level[t];
  const float* nd = R.nodes_out + (size_t)g * 32;
  float tl[3] = {INFINITY, INFINITY, INFINITY}, th[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int j = 0; j < 4; ++j) {
    const int32_t ref = __float_as_int(nd[4 * j + 3]), cnt = __float_as_int(nd[16 + 4 * j + 3]);
    if (ref < 0) continue;
    float l[3], h[3];
    const bool ok = cnt > 0 ? records_box(R.tris_out + (size_t)kTriFloats * (size_t)(R.tb + ref), cnt, l, h) : stored_box(R.tight_out + 6 * (size_t)(R.nb + ref), l, h);
    if (!ok) continue;                                                     // (the gather refused a bad record: every box is good)
    for (int a = 0; a < 3; ++a) { tl[a] = fminf(tl[a], l[a]); th[a] = fmaxf(th[a], h[a]); }
  }
  float* o = R.tight_out + 6 * (size_t)g;
  o[0] = tl[0]; o[1] = tl[1]; o[2] = tl[2]; o[3] = th[0]; o[4] = th[1]; o[5] = th[2];
}

static dim3 move_grid(int n) { return dim3((unsigned)((n + kMoveBlock - 1) / kMoveBlock)); }

void launch_move_matrices(hipStream_t st, const MoveArgs& M) {
  hipLaunchKernelGGL(k_move_begin, move_grid(M.n_mesh), dim3(kMoveBlock), 0, st, M);
  hipLaunchKernelGGL(k_move_matrices, move_grid(M.n_entry), dim3(kMoveBlock), 0, st, M);
  hipLaunchKernelGGL(k_move_pads_inst, move_grid(M.n_inst), dim3(kMoveBlock), 0, st, M);
  hipLaunchKernelGGL(k_move_pads_mesh, move_grid(M.n_mesh), dim3(kMoveBlock), 0, st, M);
}

void launch_move_repad(hipStream_t st, const MoveArgs& M) {
  hipLaunchKernelGGL(k_move_repad, move_grid(M.n_blas_nodes), dim3(kMoveBlock), 0, st, M);
}

void launch_move_entry_boxes(hipStream_t st, const MoveArgs& M, bool small) {
  if (small) hipLaunchKernelGGL(k_move_entry_boxes<64>, dim3((unsigned)M.n_entry), dim3(64), 0, st, M);
  else hipLaunchKernelGGL(k_move_entry_boxes<256>, dim3((unsigned)M.n_entry), dim3(256), 0, st, M);
}

void launch_move_tlas_level(hipStream_t st, const MoveArgs& M, const int32_t* level_nodes, int n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_move_tlas_level, move_grid(n), dim3(kMoveBlock), 0, st, M, level_nodes, n);
}

void launch_refit_mesh_level(hipStream_t st, const MoveArgs& M, const int32_t* level_nodes, int n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_refit_mesh_level, move_grid(n), dim3(kMoveBlock), 0, st, M, level_nodes, n);
}

void launch_refit_mesh_box(hipStream_t st, const MoveArgs& M, int mesh) {
  hipLaunchKernelGGL(k_refit_mesh_box, dim3(1), dim3(64), 0, st, M, mesh);
}

void launch_inst_gather(hipStream_t st, const InstRebuildArgs& R) {
  hipLaunchKernelGGL(k_inst_gather, move_grid(R.n_entry), dim3(kMoveBlock), 0, st, R);
}

void launch_inst_finish(hipStream_t st, const InstRebuildArgs& R) {
  hipLaunchKernelGGL(k_inst_finish, move_grid(R.n_tlas_new), dim3(kMoveBlock), 0, st, R);
}

void launch_inst_relocate(hipStream_t st, const InstRebuildArgs& R) {
  hipLaunchKernelGGL(k_inst_relocate, move_grid(R.n_blas_nodes > R.n_entry ? R.n_blas_nodes : R.n_entry), dim3(kMoveBlock), 0, st, R);
}

void launch_mesh_gather(hipStream_t st, const MeshRebuildArgs& R) {
  hipLaunchKernelGGL(k_mesh_gather, move_grid(R.n_recs), dim3(kMoveBlock), 0, st, R);
}

void launch_mesh_finish(hipStream_t st, const MeshRebuildArgs& R) {
  const int64_t lanes = 4 * (int64_t)(R.n_new > R.n_recs ? R.n_new : R.n_recs);
  hipLaunchKernelGGL(k_mesh_finish, dim3((unsigned)((lanes + kMoveBlock - 1) / kMoveBlock)), dim3(kMoveBlock), 0, st, R);
}

void launch_mesh_relocate(hipStream_t st, const MeshRebuildArgs& R) {
  int64_t lanes = 8 * (int64_t)R.n_blas_old;
  if (4 * ((int64_t)R.n_tlas + R.n_blas_old) > lanes) lanes = 4 * ((int64_t)R.n_tlas + R.n_blas_old);
  if (8 * (int64_t)R.n_entry > lanes) lanes = 8 * (int64_t)R.n_entry;
  hipLaunchKernelGGL(k_mesh_relocate, dim3((unsigned)((lanes + kMoveBlock - 1) / kMoveBlock)), dim3(kMoveBlock), 0, st, R);
}

void launch_mesh_tight_level(hipStream_t st, const MeshRebuildArgs& R, const int32_t* level_nodes, int n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_mesh_tight_level, move_grid(n), dim3(kMoveBlock), 0, st, R, level_nodes, n);
}

}  // namespace art
