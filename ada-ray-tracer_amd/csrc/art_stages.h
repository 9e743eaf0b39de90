// art_stages.h -- launch interface of art_stages.hip: the wavefront path-tracing stages of a render pass and the debug pass.
#pragma once
#include <hip/hip_runtime.h>
#include "art_scene.h"

namespace art {

void launch_raygen(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q);
void launch_bump(hipStream_t st, unsigned long long* a, unsigned long long* b, unsigned long long n);    // *a += n; if (b) *b += n
// end of a batch: items[b] += input items of bounce b, items[16 + b] += the items it kept (live[32 (b + 1)]); bounce 0 reads the P camera paths
void launch_acc_items(hipStream_t st, const int* live, int depth, int P, unsigned long long* items);
void launch_shade(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q, int bounce);
void launch_finish(hipStream_t st, const DevFrame& F, const DevPaths& Q, int last_level);
// compacted work sets (k_shade_compact): shade the items of Qi, write the survivors densely to Qo (+ their slot ids); n_in nullptr: all Qi.P items
// rays_a / rays_b: += the rays the stage emits as trace records (Qo.rec != nullptr); rays_b may be nullptr
void launch_shade_compact(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Qi, const DevPaths& Qo, int bounce,
                          const int* n_in, int* n_out, uint32_t* slot_out, unsigned long long* lost, unsigned long long* rays_a, unsigned long long* rays_b,
                          int per = 0, int camera_order = 0);      // per: items per thread, 2 or 0 = the default (4); camera_order: bounce 0 visits the slots tile-major (art_camera_order.h)
void launch_resolve_last(hipStream_t st, const DevPaths& Q, const int* n, int last_level);
void launch_fold(hipStream_t st, const DevFrame& F, const DevPaths& Q);
void launch_fold_levels(hipStream_t st, const DevFrame& F, const DevPaths& Q, int max_depth, const int* counts);     // dense fold records: counts[32 k] = items of level k
void launch_accumulate(hipStream_t st, const DevFrame& F, const DevPaths& Q, int samples_in_batch, float* accum);
void launch_accumulate_moments(hipStream_t st, const DevFrame& F, const DevPaths& Q, int samples_in_batch, float* accum, float* moments);   // art_bind_moments: the accum and {S1, S2} in one walk
void launch_debug(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q, float* accum, int32_t* prim_index, int32_t* mat_id, int32_t* prim_type);

}  // namespace art
