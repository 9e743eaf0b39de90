// art_tree_walk.h -- host only, no HIP: what every host-side reader of wide-node packets shares.  slot_words unpacks a slot; walk_levels
// groups a tree's nodes by depth and checks on the way that the packets form a tree -- the check that decides whether kernels may be
// launched over a tree read back from HBM (art_update.cpp's refit plan, art_instanced_build.cpp's move plan, art_renumber.h).
// tests/tree_walk_check.cpp tests both on the CPU.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace art {

// slot j of a packet of `width` slots (8 * width floats): ref < 0: empty; cnt > 0: a leaf of cnt records from ref; else an inner child
inline void slot_words(const float* packet, int width, int j, int32_t& ref, int32_t& cnt) {
  std::memcpy(&ref, packet + 4 * j + 3, 4); std::memcpy(&cnt, packet + 4 * width + 4 * j + 3, 4);
}

enum class TreeFault { none = 0, leaf_outside_records = 1, child_out_of_range_or_twice = 2, unreachable_nodes = 3 };      // (a call site's messages are indexed by it)

// Breadth first from the root `base` over the n_nodes packets nodes[base .. base + n_nodes): a child reference is relative to base and
// must name one of them, each at most once, and all of them must be reached.  A leaf holds at most max_leaf records and ends inside
// n_recs of them (n_recs < 0: leaves are not bounded).  visit(node) runs on every node as it is first reached.  Appended to `levels`:
// the nodes' numbers in `nodes`, parents in level order, children in slot order; to `level_off` (which starts as {0} when it is empty):
// where every level ends in `levels`.
template <typename Visit>
inline TreeFault walk_levels(const float* nodes, int width, int64_t base, int64_t n_nodes, int64_t n_recs, int max_leaf, std::vector<int32_t>& levels,
                             std::vector<int>& level_off, Visit&& visit) {
  if (n_nodes < 1) return TreeFault::unreachable_nodes;
  const size_t first = levels.size();
  std::vector<uint8_t> seen((size_t)n_nodes, 0);
  if (level_off.empty()) level_off.push_back(0);
  seen[0] = 1; levels.push_back((int32_t)base); visit((int32_t)base);
  for (size_t b = first; b < levels.size();) {
    const size_t e = levels.size();
    for (size_t i = b; i < e; ++i)
      for (int j = 0; j < width; ++j) {
        int32_t ref, cnt;
        slot_words(nodes + (size_t)levels[i] * 8 * (size_t)width, width, j, ref, cnt);
        if (ref < 0) continue;
        if (cnt > 0) {
          if (n_recs >= 0 && (cnt > max_leaf || (int64_t)ref + cnt > n_recs)) return TreeFault::leaf_outside_records;
          continue;
        }
        if (ref >= n_nodes || seen[(size_t)ref]) return TreeFault::child_out_of_range_or_twice;
        seen[(size_t)ref] = 1; levels.push_back((int32_t)(base + ref)); visit((int32_t)(base + ref));
      }
    level_off.push_back((int)e);
    b = e;
  }
  return (int64_t)(levels.size() - first) == n_nodes ? TreeFault::none : TreeFault::unreachable_nodes;
}

}  // namespace art
