// art_renumber.h -- host only, no HIP: a 4-wide tree as a GPU builder left it (any numbering of its nodes, a leaf's records lying one
// after the other) -> the numbering the host builder gives the same tree.  art_bvh.cpp's collapse takes a node's slots in order, gives
// every leaf's records and every inner child the next free number, and goes on with the child it numbered last.  Inside a leaf the
// records keep their order.  The tree is checked on the way, as build_move_plan_host checks a build: every node reached exactly once,
// every record named by exactly one leaf.  art_update.cpp uses it for the instance tree (one record per leaf) and for a mesh's tree
// (1 to kMaxLeafTris records); tests/renumber_check.cpp tests it on the CPU.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "art_tree_walk.h"

namespace art {

// nodes: N packets of 32 floats (slot j: ref = word 4 j + 3, count = word 16 + 4 j + 3; ref < 0: empty; count 0: an inner child).
// node_map[builder's node] / rec_map[builder's record] = the host builder's number.  levels: the nodes by depth, root first, in the NEW
// numbering; level L = levels[level_off[L] .. level_off[L + 1]).  what: the tree's name in a message.
inline bool renumber_built_tree(const float* nodes, int64_t N, int64_t n_recs, int max_leaf, const std::string& what, std::vector<int32_t>& node_map,
                                std::vector<int32_t>& rec_map, std::vector<int32_t>& levels, std::vector<int>& level_off, std::string& err) {
  if (N < 1 || N > 0x7fffffff || n_recs < 0 || n_recs > 0x7fffffff) { err = "the built " + what + " is empty or too large"; return false; }
  levels.clear(); level_off.clear();                                       // (walked in the builder's numbers; the levels hold the new ones below)
  const TreeFault fault = walk_levels(nodes, 4, 0, N, n_recs, max_leaf, levels, level_off, [](int32_t) {});
  if (fault == TreeFault::leaf_outside_records) { err = "the built " + what + " has a leaf outside its records"; return false; }
  if (fault == TreeFault::child_out_of_range_or_twice) { err = "the built " + what + "'s nodes do not form a tree"; return false; }
  if (fault == TreeFault::unreachable_nodes) { err = "unreachable nodes in the built " + what; return false; }
  node_map.assign((size_t)N, -1); rec_map.assign((size_t)n_recs, -1);
  std::vector<int32_t> todo(1, 0);
  int32_t next_node = 1, next_rec = 0;
  node_map[0] = 0;
  while (!todo.empty()) {                                                  // (a tree, and every leaf inside the records: the walk has checked it)
    const int32_t n = todo.back(); todo.pop_back();
    for (int j = 0; j < 4; ++j) {
      int32_t ref, cnt;
      slot_words(nodes + (size_t)n * 32, 4, j, ref, cnt);
      if (ref < 0) continue;
      if (cnt < 0) { err = "the built " + what + " has a leaf outside its records"; return false; }
      if (cnt == 0) { node_map[(size_t)ref] = next_node++; todo.push_back(ref); continue; }
      for (int32_t r = 0; r < cnt; ++r) {
        if (rec_map[(size_t)ref + (size_t)r] >= 0) { err = "a record of the built " + what + " is named twice"; return false; }
        rec_map[(size_t)ref + (size_t)r] = next_rec++;
      }
    }
  }
  if (next_rec != n_recs) { err = "a record without a leaf in the built " + what; return false; }
  for (int32_t& n : levels) n = node_map[(size_t)n];
  return true;
}

}  // namespace art
