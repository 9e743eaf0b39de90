// art_renumber.h -- host only, no HIP: a 4-wide tree as a GPU builder left it (any numbering of its nodes, a leaf's records lying one
// after the other) -> the numbering the host builder gives the same tree.  art_bvh.cpp's collapse takes a node's slots in order, gives
// every leaf's records and every inner child the next free number, and goes on with the child it numbered last.  Inside a leaf the
// records keep their order.  The tree is checked on the way, as build_move_plan_host checks a build: every node reached exactly once,
// every record named by exactly one leaf.  art_update.cpp uses it for the instance tree (one record per leaf) and for a mesh's tree
// (1 to kMaxLeafTris records); tests/renumber_check.cpp tests it on the CPU.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace art {

// nodes: N packets of 32 floats (slot j: ref = word 4 j + 3, count = word 16 + 4 j + 3; ref < 0: empty; count 0: an inner child).
// node_map[builder's node] / rec_map[builder's record] = the host builder's number.  levels: the nodes by depth, root first, in the NEW
// numbering; level L = levels[level_off[L] .. level_off[L + 1]).  what: the tree's name in a message.
inline bool renumber_built_tree(const float* nodes, int64_t N, int64_t n_recs, int max_leaf, const std::string& what, std::vector<int32_t>& node_map,
                                std::vector<int32_t>& rec_map, std::vector<int32_t>& levels, std::vector<int>& level_off, std::string& err) {
  if (N < 1 || N > 0x7fffffff || n_recs < 0 || n_recs > 0x7fffffff) { err = "the built " + what + " is empty or too large"; return false; }
  node_map.assign((size_t)N, -1); rec_map.assign((size_t)n_recs, -1);
  auto words = [&](int32_t n, int j, int32_t& ref, int32_t& cnt) { std::memcpy(&ref, &nodes[(size_t)n * 32 + 4 * j + 3], 4); std::memcpy(&cnt, &nodes[(size_t)n * 32 + 16 + 4 * j + 3], 4); };
  std::vector<int32_t> todo(1, 0);
  int64_t next_node = 1, next_rec = 0;
  node_map[0] = 0;
  while (!todo.empty()) {
    const int32_t n = todo.back(); todo.pop_back();
    for (int j = 0; j < 4; ++j) {
      int32_t ref, cnt;
      words(n, j, ref, cnt);
      if (ref < 0) continue;
      if (cnt != 0) {
        if (cnt < 1 || cnt > max_leaf || (int64_t)ref + cnt > n_recs) { err = "the built " + what + " has a leaf outside its records"; return false; }
        for (int32_t r = 0; r < cnt; ++r) {
          if (rec_map[(size_t)ref + (size_t)r] >= 0) { err = "a record of the built " + what + " is named twice"; return false; }
          rec_map[(size_t)ref + (size_t)r] = (int32_t)next_rec++;
        }
        continue;
      }
      if (ref >= N || node_map[(size_t)ref] >= 0) { err = "the built " + what + "'s nodes do not form a tree"; return false; }
      node_map[(size_t)ref] = (int32_t)next_node++; todo.push_back(ref);
    }
  }
  if (next_node != N) { err = "unreachable nodes in the built " + what; return false; }
  if (next_rec != n_recs) { err = "a record without a leaf in the built " + what; return false; }
  std::vector<int32_t> cur(1, 0), next;                                    // (the builder's numbers; the levels hold the new ones)
  levels.clear(); level_off.assign(1, 0);
  while (!cur.empty()) {
    next.clear();
    for (const int32_t n : cur) {
      levels.push_back(node_map[(size_t)n]);
      for (int j = 0; j < 4; ++j) { int32_t ref, cnt; words(n, j, ref, cnt); if (ref >= 0 && cnt == 0) next.push_back(ref); }
    }
    level_off.push_back((int)levels.size());
    cur.swap(next);
  }
  return true;
}

}  // namespace art
