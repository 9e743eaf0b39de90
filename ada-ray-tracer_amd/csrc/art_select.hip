// art_select.hip -- the gfx950 kernels of art_compact_mask_device and of the masked render pass (art_render_pass_masked): ordered stream
// compaction of a byte mask over the rank's pixel list, and the per-pixel sample counts of a masked pass.
//
// The list has n entries (pixmap[i], the rank's pixels in tile order); entry i is SELECTED when mask[pixmap[i]] != 0.  The output holds
// the selected entries in list order.  Workgroups of 256 lanes (4 waves of 64) take 256 consecutive entries each, and THREE launches
// combine them; no workgroup ever waits for another one (no flag is polled, no atomic decides a position), so the result is the same
// bytes on every run and nothing can hang on a lost wake-up:
//
//   k_select_count    block b counts its selected entries: one __ballot per wave (a 64-bit mask), its popcount into LDS, the four wave
//                     counts summed -> block_sums[b].  Reads 4 bytes of pixmap (contiguous, 1 KB per workgroup) and 1 byte of mask per
//                     entry; inside a 32 x 32 tile the 32 entries of a tile row are 32 contiguous bytes of the mask.
//   k_select_scan     ONE workgroup turns block_sums into their exclusive prefix sums in place, 256 blocks per step with a running carry
//                     (any number of blocks: 2^28 entries are 2^20 blocks, 4096 steps), and writes the total to *count_out.  Per step a
//                     wave scans its 64 values with __shfl_up, the wave totals go through LDS.
//   k_select_scatter  block b repeats k_select_count's ballots; an entry's position is block_sums[b] + the counts of the waves before its
//                     own + the popcount of its wave's ballot below its lane.  A wave's stores are contiguous.
//
// Compulsory bytes: count reads 5 n, scatter reads 5 n again (the mask lines may still be in L2) and writes 4 x selected; the scan moves
// 8 bytes per block.  EXPECTATION, not yet measured (profiles/adaptive/measure.py is the script): at 1920 x 1080 each launch is at its
// launch cost of a few microseconds, far above its byte floor of 1.6 / 0.01 / 3.3 us at 6.3 TB/s.
//
//   k_add_counts      counts[list[i]] += samples for the n entries of a compacted list: the entries are distinct, so every word has one
//                     writer.
#include <hip/hip_runtime.h>
#include "art_select.h"

namespace art {

constexpr int kSelBlock = 256, kSelWaves = kSelBlock / 64;

// every lane of the workgroup calls this (it holds a barrier).  Returns the number of selected lanes before this one in the workgroup;
// total = the workgroup's count.
__device__ __forceinline__ int block_rank(bool sel, int& total) {
  __shared__ int wave_count[kSelWaves];
  const unsigned long long b = __ballot(sel);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_count[wave] = __popcll(b);
  __syncthreads();
  int before = 0; total = 0;
#pragma unroll
  for (int w = 0; w < kSelWaves; ++w) { const int c = wave_count[w]; total += c; if (w < wave) before += c; }
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kSelBlock) void k_select_count(const SelectArgs A) {
  const int i = blockIdx.x * kSelBlock + threadIdx.x;            // at most 2^28 entries (the host's bound)
  const bool sel = i < A.n && A.mask[A.pixmap[i]] != 0;
  int total;
  (void)block_rank(sel, total);
  if (threadIdx.x == 0) A.block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(kSelBlock) void k_select_scan(uint32_t* block_sums, int n_blocks, uint32_t* count_out) {
  __shared__ uint32_t wave_total[kSelWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (int base = 0; base < n_blocks; base += kSelBlock) {
    const int j = base + (int)threadIdx.x;
    const uint32_t v = j < n_blocks ? block_sums[j] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d); if (lane >= d) incl += up; }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSelWaves; ++w) { const uint32_t c = wave_total[w]; total += c; if (w < wave) before += c; }
    if (j < n_blocks) block_sums[j] = carry + before + (incl - v);
    carry += total;
    __syncthreads();                                             // (wave_total is written again in the next step)
  }
  if (threadIdx.x == 0) *count_out = carry;
}

__global__ __launch_bounds__(kSelBlock) void k_select_scatter(const SelectArgs A) {
  const int i = blockIdx.x * kSelBlock + threadIdx.x;
  const uint32_t g = i < A.n ? A.pixmap[i] : 0u;
  const bool sel = i < A.n && A.mask[g] != 0;
  int total;
  const int rank = block_rank(sel, total);
  if (sel) A.out[A.block_sums[blockIdx.x] + (uint32_t)rank] = g;
}

__global__ __launch_bounds__(kSelBlock) void k_add_counts(const uint32_t* list, int n, uint32_t* counts, uint32_t samples) {
  const int i = blockIdx.x * kSelBlock + threadIdx.x;
  if (i < n) counts[list[i]] += samples;
}

int select_blocks(int n) { return (n + kSelBlock - 1) / kSelBlock; }

void launch_compact_mask(hipStream_t st, const SelectArgs& A, uint32_t* count_out) {
  const int blocks = select_blocks(A.n);
  hipLaunchKernelGGL(k_select_count, dim3((unsigned)blocks), dim3(kSelBlock), 0, st, A);
  hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(kSelBlock), 0, st, A.block_sums, blocks, count_out);
  hipLaunchKernelGGL(k_select_scatter, dim3((unsigned)blocks), dim3(kSelBlock), 0, st, A);
}

void launch_add_counts(hipStream_t st, const uint32_t* list, int n, uint32_t* counts, uint32_t samples) {
  hipLaunchKernelGGL(k_add_counts, dim3((unsigned)select_blocks(n)), dim3(kSelBlock), 0, st, list, n, counts, samples);
}

}  // namespace art
