// TEST-ONLY: the renumbering of a GPU-built tree into the host builder's numbering (csrc/art_renumber.h) against the host builder
// itself.  The host builder's 4-wide tree of a mesh is taken, its node numbers and the order of its leaves' record runs are shuffled
// (references fixed), and the renumbering must give the original arrays back byte for byte.  Trees that are no trees must be refused.
// Built as a stand-alone program (tests/test_renumber.py), also with AddressSanitizer + UBSan.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../ada-ray-tracer_amd/csrc/art_bvh.h"
#include "../ada-ray-tracer_amd/csrc/art_renumber.h"

using namespace art;

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_seed >> 33); }
static float rndf() { return (float)(rnd() & 0xffffff) / 16777216.0f; }

static int32_t word(const std::vector<float>& v, size_t i) { int32_t w; std::memcpy(&w, &v[i], 4); return w; }
static void set_word(std::vector<float>& v, size_t i, int32_t w) { std::memcpy(&v[i], &w, 4); }

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

// the shuffled tree: nodes[perm[i]] = node i (the root stays node 0), the leaves' record runs in a shuffled order
static void shuffle_tree(const Bvh8& b, std::vector<float>& nodes, std::vector<float>& tris) {
  const int32_t N = b.n_nodes;
  std::vector<int32_t> perm((size_t)N);
  std::iota(perm.begin(), perm.end(), 0);
  for (int32_t i = N - 1; i > 1; --i) std::swap(perm[(size_t)i], perm[(size_t)(1 + rnd() % (uint32_t)i)]);
  struct Run { int32_t node, slot, ref, cnt; };
  std::vector<Run> runs;
  for (int32_t n = 0; n < N; ++n)
    for (int j = 0; j < 4; ++j) {
      const int32_t ref = word(b.nodes, (size_t)n * 32 + 4 * j + 3), cnt = word(b.nodes, (size_t)n * 32 + 16 + 4 * j + 3);
      if (ref >= 0 && cnt > 0) runs.push_back(Run{n, j, ref, cnt});
    }
  for (size_t i = runs.size(); i > 1; --i) std::swap(runs[i - 1], runs[rnd() % i]);
  nodes.assign(b.nodes.size(), 0.0f); tris.assign(b.tris.size(), 0.0f);
  std::vector<float> moved = b.nodes;
  int32_t at = 0;
  for (const Run& r : runs) {
    std::memcpy(&tris[(size_t)at * kTriFloats], &b.tris[(size_t)r.ref * kTriFloats], (size_t)r.cnt * kTriFloats * 4);
    set_word(moved, (size_t)r.node * 32 + 4 * r.slot + 3, at);
    at += r.cnt;
  }
  for (int32_t n = 0; n < N; ++n) {
    for (int j = 0; j < 4; ++j) {
      const int32_t ref = word(moved, (size_t)n * 32 + 4 * j + 3), cnt = word(moved, (size_t)n * 32 + 16 + 4 * j + 3);
      if (ref >= 0 && cnt == 0) set_word(moved, (size_t)n * 32 + 4 * j + 3, perm[(size_t)ref]);
    }
    std::memcpy(&nodes[(size_t)perm[(size_t)n] * 32], &moved[(size_t)n * 32], 128);
  }
}

static int one_mesh(int n, std::vector<float>* keep_nodes, int32_t* keep_recs) {
  std::vector<float> tri9((size_t)n * 9);
  for (int t = 0; t < n; ++t) {
    const float c[3] = {rndf() * 10.0f, rndf() * 10.0f, rndf() * 10.0f};
    for (int k = 0; k < 9; ++k) tri9[(size_t)t * 9 + k] = c[k % 3] + 0.3f * (rndf() - 0.5f);
  }
  BvhBuildParams bp; bp.width = 4;
  Bvh8 b; std::string err;
  CHECK(build_bvh8(tri9.data(), nullptr, n, bp, b, err), "build_bvh8(%d): %s", n, err.c_str());
  CHECK(b.n_tris == n && b.n_nodes >= 1, "build_bvh8(%d): sizes", n);
  for (int round = 0; round < 3; ++round) {
    std::vector<float> nodes, tris;
    shuffle_tree(b, nodes, tris);
    std::vector<int32_t> node_map, rec_map, levels; std::vector<int> level_off;
    CHECK(renumber_built_tree(nodes.data(), b.n_nodes, n, 4, "test tree", node_map, rec_map, levels, level_off, err), "renumber(%d): %s", n, err.c_str());
    std::vector<float> out_nodes(nodes.size()), out_tris(tris.size());
    for (int32_t i = 0; i < b.n_nodes; ++i) {
      std::vector<float> nd(nodes.begin() + (size_t)i * 32, nodes.begin() + (size_t)i * 32 + 32);
      for (int j = 0; j < 4; ++j) {
        const int32_t ref = word(nd, 4 * j + 3), cnt = word(nd, 16 + 4 * j + 3);
        if (ref >= 0) set_word(nd, 4 * j + 3, cnt ? rec_map[(size_t)ref] : node_map[(size_t)ref]);
      }
      std::memcpy(&out_nodes[(size_t)node_map[(size_t)i] * 32], nd.data(), 128);
    }
    for (int32_t r = 0; r < n; ++r) std::memcpy(&out_tris[(size_t)rec_map[(size_t)r] * kTriFloats], &tris[(size_t)r * kTriFloats], kTriFloats * 4);
    CHECK(std::memcmp(out_nodes.data(), b.nodes.data(), b.nodes.size() * 4) == 0, "n = %d round %d: the renumbered nodes are not the host builder's", n, round);
    CHECK(std::memcmp(out_tris.data(), b.tris.data(), b.tris.size() * 4) == 0, "n = %d round %d: the renumbered records are not the host builder's", n, round);
    // the levels: breadth first over the ORIGINAL tree
    std::vector<int32_t> want, cur(1, 0), next; std::vector<int> want_off(1, 0);
    while (!cur.empty()) {
      next.clear();
      for (const int32_t g : cur) {
        want.push_back(g);
        for (int j = 0; j < 4; ++j) { const int32_t ref = word(b.nodes, (size_t)g * 32 + 4 * j + 3), cnt = word(b.nodes, (size_t)g * 32 + 16 + 4 * j + 3); if (ref >= 0 && cnt == 0) next.push_back(ref); }
      }
      want_off.push_back((int)want.size());
      cur.swap(next);
    }
    CHECK(level_off == want_off, "n = %d: level offsets", n);
    for (size_t L = 0; L + 1 < want_off.size(); ++L) {               // (a level is a set: the shuffled slots' order is the same, the walk order too)
      std::vector<int32_t> a(levels.begin() + want_off[L], levels.begin() + want_off[L + 1]), w(want.begin() + want_off[L], want.begin() + want_off[L + 1]);
      std::sort(a.begin(), a.end()); std::sort(w.begin(), w.end());
      CHECK(a == w, "n = %d: level %zu", n, L);
    }
    if (keep_nodes && round == 0) { *keep_nodes = nodes; *keep_recs = n; }
  }
  return 0;
}

int main() {
  std::vector<float> nodes; int32_t n_recs = 0;
  for (const int n : {2, 5, 300, 2000}) if (one_mesh(n, n == 300 ? &nodes : nullptr, &n_recs)) return 1;
  const int64_t N = (int64_t)(nodes.size() / 32);
  std::vector<int32_t> node_map, rec_map, levels; std::vector<int> level_off; std::string err;
  CHECK(N > 4 && renumber_built_tree(nodes.data(), N, n_recs, 4, "test tree", node_map, rec_map, levels, level_off, err), "the kept tree: %s", err.c_str());
  // inner slots and leaf slots of the kept tree
  std::vector<size_t> inner, leaf;
  for (int64_t n = 0; n < N; ++n)
    for (int j = 0; j < 4; ++j) {
      const int32_t ref = word(nodes, (size_t)n * 32 + 4 * j + 3), cnt = word(nodes, (size_t)n * 32 + 16 + 4 * j + 3);
      if (ref >= 0) (cnt ? leaf : inner).push_back((size_t)n * 32 + 4 * j + 3);
    }
  CHECK(inner.size() >= 2 && leaf.size() >= 2, "the kept tree is too small");
  {                                                                        // a node reached twice
    std::vector<float> bad = nodes;
    set_word(bad, inner[1], word(bad, inner[0]));
    CHECK(!renumber_built_tree(bad.data(), N, n_recs, 4, "test tree", node_map, rec_map, levels, level_off, err), "a node reached twice was accepted");
  }
  {                                                                        // the root reached from below
    std::vector<float> bad = nodes;
    set_word(bad, inner[0], 0);
    CHECK(!renumber_built_tree(bad.data(), N, n_recs, 4, "test tree", node_map, rec_map, levels, level_off, err), "a cycle through the root was accepted");
  }
  {                                                                        // an unreachable node
    std::vector<float> bad = nodes;
    set_word(bad, inner[0], -1);
    CHECK(!renumber_built_tree(bad.data(), N, n_recs, 4, "test tree", node_map, rec_map, levels, level_off, err) && err.find("unreachable") != std::string::npos, "an unreachable node was accepted: %s", err.c_str());
  }
  {                                                                        // a record named twice
    std::vector<float> bad = nodes;
    set_word(bad, leaf[1], word(bad, leaf[0]));
    CHECK(!renumber_built_tree(bad.data(), N, n_recs, 4, "test tree", node_map, rec_map, levels, level_off, err), "a record named twice was accepted");
  }
  {                                                                        // a leaf beyond the records, a leaf too large, a node beyond the array
    std::vector<float> bad = nodes;
    set_word(bad, leaf[0], n_recs);
    CHECK(!renumber_built_tree(bad.data(), N, n_recs, 4, "test tree", node_map, rec_map, levels, level_off, err), "a leaf outside the records was accepted");
    bad = nodes; set_word(bad, leaf[0] + 16, 5);
    CHECK(!renumber_built_tree(bad.data(), N, n_recs, 4, "test tree", node_map, rec_map, levels, level_off, err), "a leaf of five records was accepted");
    bad = nodes; set_word(bad, inner[0], (int32_t)N);
    CHECK(!renumber_built_tree(bad.data(), N, n_recs, 4, "test tree", node_map, rec_map, levels, level_off, err), "a node outside the array was accepted");
  }
  std::printf("renumber ok\n");
  return 0;
}
