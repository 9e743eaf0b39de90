// TEST-ONLY: the one breadth-first walk over wide-node packets (csrc/art_tree_walk.h).  Hand-made packets at the smallest shapes that can go
// wrong, every malformation on its own, and the walk's three users' levels -- the move plan of a two-level build of two meshes and three
// instances (art_instanced_build.cpp) and the refit walk's input at widths 4 and 8 (the host builder's trees, art_bvh.cpp) -- against
// levels derived a different way: every node's depth by recursion from its root, the nodes grouped by depth, inside a depth in the order of
// first reach.  The derivation reads the packets with its own memcpy, not with slot_words.  Built as a stand-alone program
// (tests/test_renumber.py), also with AddressSanitizer + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ada-ray-tracer_amd/csrc/art_bvh.h"
#include "../ada-ray-tracer_amd/csrc/art_instanced_build.h"
#include "../ada-ray-tracer_amd/csrc/art_tree_walk.h"

using namespace art;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static float rndf() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (float)((uint32_t)(g_seed >> 33) & 0xffffff) / 16777216.0f; }

struct Slot { int32_t ref, cnt; };
using Packets = std::vector<std::vector<Slot>>;          // per node its used slots; cnt 0: an inner child

static std::vector<float> make_nodes(int W, const Packets& p) {
  std::vector<float> nodes(p.size() * 8 * (size_t)W, 0.0f);
  for (size_t n = 0; n < p.size(); ++n)
    for (int j = 0; j < W; ++j) {
      const Slot s = (size_t)j < p[n].size() ? p[n][(size_t)j] : Slot{-1, 0};
      std::memcpy(&nodes[n * 8 * W + 4 * j + 3], &s.ref, 4); std::memcpy(&nodes[n * 8 * W + 4 * W + 4 * j + 3], &s.cnt, 4);
    }
  return nodes;
}

struct Walk { TreeFault fault; std::vector<int32_t> levels, visited; std::vector<int> off; };
static Walk walk(const std::vector<float>& nodes, int W, int64_t base, int64_t n_nodes, int64_t n_recs, int max_leaf) {
  Walk w;
  w.fault = walk_levels(nodes.data(), W, base, n_nodes, n_recs, max_leaf, w.levels, w.off, [&](int32_t n) { w.visited.push_back(n); });
  return w;
}

// the other way: depth by recursion, grouped by depth, in the order of first reach
static void by_depth(const float* nodes, int W, int64_t base, int32_t node, size_t depth, std::vector<std::vector<int32_t>>& at) {
  if (at.size() <= depth) at.resize(depth + 1);
  at[depth].push_back(node);
  for (int j = 0; j < W; ++j) {
    int32_t ref, cnt;
    std::memcpy(&ref, nodes + (size_t)node * 8 * W + 4 * j + 3, 4); std::memcpy(&cnt, nodes + (size_t)node * 8 * W + 4 * W + 4 * j + 3, 4);
    if (ref >= 0 && cnt <= 0) by_depth(nodes, W, base, (int32_t)(base + ref), depth + 1, at);
  }
}
static void append_levels(const float* nodes, int W, int64_t root, std::vector<int32_t>& levels, std::vector<int>& off) {
  std::vector<std::vector<int32_t>> at;
  by_depth(nodes, W, root, (int32_t)root, 0, at);
  if (off.empty()) off.push_back(0);
  for (const std::vector<int32_t>& l : at) { levels.insert(levels.end(), l.begin(), l.end()); off.push_back((int)levels.size()); }
}

static int hand_made() {
  for (const int W : {4, 8}) {
    {                                                                      // a root whose only slot is a leaf
      const Walk w = walk(make_nodes(W, {{{0, 1}}}), W, 0, 1, 1, 1);
      CHECK(w.fault == TreeFault::none && w.levels == std::vector<int32_t>{0} && w.off == (std::vector<int>{0, 1}) && w.visited == w.levels, "W %d: a root with one leaf", W);
    }
    // three levels, numbered against the walk's order: 0 -> {2, leaf, 1}, 2 -> {leaf, 3}, 1 -> {leaf}, 3 -> {leaf, leaf}
    const Packets three = {{{2, 0}, {0, 2}, {1, 0}}, {{2, 1}}, {{3, 2}, {3, 0}}, {{5, 1}, {6, 2}}};
    {
      const Walk w = walk(make_nodes(W, three), W, 0, 4, 8, 2);
      CHECK(w.fault == TreeFault::none && w.levels == (std::vector<int32_t>{0, 2, 1, 3}) && w.off == (std::vector<int>{0, 1, 3, 4}) && w.visited == w.levels, "W %d: three levels", W);
    }
    {                                                                      // the same tree at base 2 of a larger array, appended to what the vectors hold
      Packets big = {{{0, 1}}, {{0, 1}}};
      big.insert(big.end(), three.begin(), three.end());
      big.push_back({{0, 1}});
      const std::vector<float> nodes = make_nodes(W, big);
      std::vector<int32_t> levels = {0, 1}; std::vector<int> off = {0, 1, 2}, seen;
      CHECK(walk_levels(nodes.data(), W, 2, 4, 8, 2, levels, off, [&](int32_t n) { seen.push_back(n); }) == TreeFault::none, "W %d: a subtree at base 2", W);
      CHECK(levels == (std::vector<int32_t>{0, 1, 2, 4, 3, 5}) && off == (std::vector<int>{0, 1, 2, 3, 5, 6}) && seen == (std::vector<int32_t>{2, 4, 3, 5}), "W %d: a subtree's levels", W);
      big[2][0].ref = 4;                                                   // the bound of the subtree, though the array holds that node
      big[5] = {{0, 1}};
      CHECK(walk(make_nodes(W, big), W, 2, 4, 8, 2).fault == TreeFault::child_out_of_range_or_twice, "W %d: a child at the subtree's bound", W);
    }
    {                                                                      // leaves are not bounded
      Packets p = three; p[1][0] = {1000000, 9};
      CHECK(walk(make_nodes(W, p), W, 0, 4, -1, 2).fault == TreeFault::none, "W %d: unbounded leaves", W);
      CHECK(walk(make_nodes(W, p), W, 0, 4, 8, 2).fault == TreeFault::leaf_outside_records, "W %d: the same leaves, bounded", W);
    }
    // every malformation on its own
    { Packets p = three; p[0][0].ref = 4; CHECK(walk(make_nodes(W, p), W, 0, 4, 8, 2).fault == TreeFault::child_out_of_range_or_twice, "W %d: a child equal to the bound", W); }
    { Packets p = three; p[2][1].ref = 1; CHECK(walk(make_nodes(W, p), W, 0, 4, 8, 2).fault == TreeFault::child_out_of_range_or_twice, "W %d: a child named twice, another unreachable", W); }
    { Packets p = three; p[0][2].ref = 0; CHECK(walk(make_nodes(W, p), W, 0, 4, 8, 2).fault == TreeFault::child_out_of_range_or_twice, "W %d: the root named from below", W); }
    { Packets p = three; p[2][1] = {7, 1}; CHECK(walk(make_nodes(W, p), W, 0, 4, 8, 2).fault == TreeFault::unreachable_nodes, "W %d: a node no one names", W); }
    { Packets p = three; p[3][1].cnt = 3; CHECK(walk(make_nodes(W, p), W, 0, 4, 9, 2).fault == TreeFault::leaf_outside_records, "W %d: cnt > max_leaf", W); }
    { Packets p = three; p[3][1].ref = 7; CHECK(walk(make_nodes(W, p), W, 0, 4, 8, 2).fault == TreeFault::leaf_outside_records, "W %d: a leaf one past the records", W); }
    { Packets p = three; p[3][1].ref = 7; CHECK(walk(make_nodes(W, p), W, 0, 4, 9, 2).fault == TreeFault::none, "W %d: a leaf that ends with the records", W); }
    {                                                                      // slot_words: bit copies of word 4 j + 3 and word 4 W + 4 j + 3
      const std::vector<float> nodes = make_nodes(W, {{{-1, 0}, {0x7fc00001, (int32_t)0x80000000u}}});
      int32_t ref = 0, cnt = 0;
      slot_words(nodes.data(), W, 1, ref, cnt);
      CHECK(ref == 0x7fc00001 && cnt == (int32_t)0x80000000u, "W %d: slot_words", W);
    }
  }
  return 0;
}

static std::vector<float> soup(int n) {
  std::vector<float> tri9((size_t)n * 9);
  for (int t = 0; t < n; ++t) {
    const float c[3] = {rndf() * 10.0f, rndf() * 10.0f, rndf() * 10.0f};
    for (int k = 0; k < 9; ++k) tri9[(size_t)t * 9 + k] = c[k % 3] + 0.3f * (rndf() - 0.5f);
  }
  return tri9;
}

// the refit walk's input: the host builder's tree of the 300-triangle mesh
static int refit_input(int W) {
  const std::vector<float> tri9 = soup(300);
  BvhBuildParams bp; bp.width = W;
  Bvh8 b; std::string err;
  CHECK(build_bvh8(tri9.data(), nullptr, 300, bp, b, err), "build_bvh8 width %d: %s", W, err.c_str());
  const Walk w = walk(b.nodes, W, 0, b.n_nodes, b.n_tris, kMaxLeafTris);
  std::vector<int32_t> levels; std::vector<int> off;
  append_levels(b.nodes.data(), W, 0, levels, off);
  CHECK(w.fault == TreeFault::none && b.n_nodes > W && off.size() > 3, "width %d: the host builder's tree was refused, or is too small", W);
  CHECK(w.levels == levels && w.off == off && w.visited == levels, "width %d: the refit walk's levels", W);
  return 0;
}

// two meshes (2 and 300 triangles), three instances
static int move_plan() {
  const int nt[2] = {2, 300};
  std::vector<float> verts[2]; std::vector<int32_t> idx[2];
  std::vector<InstMeshIn> meshes;
  for (int m = 0; m < 2; ++m) {
    verts[m] = soup(nt[m]);
    for (int k = 0; k < 3 * nt[m]; ++k) idx[m].push_back(k);
    meshes.push_back(InstMeshIn{verts[m].data(), (size_t)3 * nt[m], idx[m].data(), (size_t)nt[m]});
  }
  std::vector<InstIn> insts;
  for (int i = 0; i < 3; ++i) {
    InstIn in; in.mesh = i == 0 ? 0 : 1;
    const float m[12] = {1, 0, 0, 20.0f * i, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(in.m, m, sizeof m);
    insts.push_back(in);
  }
  TwoLevelHost T; MovePlanHost P; std::string err;
  CHECK(build_two_level_host(meshes, insts, T, err, /*two_sided=*/false), "build_two_level_host: %s", err.c_str());
  CHECK(build_move_plan_host(T, P, err), "build_move_plan_host: %s", err.c_str());
  std::vector<int32_t> levels, node_mesh(T.blas_nodes.size() / 32, -1); std::vector<int> off, first(1, 0);
  for (size_t m = 0; m < 2; ++m) {
    const size_t before = levels.size();
    append_levels(T.blas_nodes.data(), 4, P.mesh_base[3 * m], levels, off);
    for (size_t k = before; k < levels.size(); ++k) node_mesh[(size_t)levels[k]] = (int32_t)m;
    first.push_back((int)off.size() - 1);
  }
  CHECK(P.blas_levels == levels && P.blas_level_off == off && P.mesh_level_first == first && P.node_mesh == node_mesh, "the meshes' levels");
  CHECK(first[2] - first[1] > 2 && first[1] == 1, "the meshes' trees: one level, and more than two");
  levels.clear(); off.clear();
  append_levels(T.tlas.nodes.data(), 4, 0, levels, off);
  CHECK(P.tlas_levels == levels && P.tlas_level_off == off && (int64_t)levels.size() == T.tlas.n_nodes, "the instance tree's levels");
  return 0;
}

int main() {
  if (hand_made() || refit_input(4) || refit_input(8) || move_plan()) return 1;
  std::printf("tree walk ok\n");
  return 0;
}
