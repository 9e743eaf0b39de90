// art_select.h -- launch interface of art_select.hip: mask compaction and the sample counts of a masked render pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace art {

// art_compact_mask_device and the masked render pass (art_select.hip): the n entries of a pixel list, the frame's byte mask, one word per
// workgroup of 256 entries (select_blocks(n) words of scratch: counts, then their exclusive prefix sums) and the compacted list
struct SelectArgs {
  const uint8_t* mask; const uint32_t* pixmap; int32_t n;
  uint32_t* block_sums; uint32_t* out;
};
int select_blocks(int n);
void launch_compact_mask(hipStream_t st, const SelectArgs& A, uint32_t* count_out);      // three launches: count, scan (one workgroup), scatter
void launch_add_counts(hipStream_t st, const uint32_t* list, int n, uint32_t* counts, uint32_t samples);   // counts[list[i]] += samples, i < n

}  // namespace art
