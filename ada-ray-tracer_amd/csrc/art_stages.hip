// art_stages.hip -- gfx950 (CDNA4, wave64): the wavefront path-tracing stages between two trace launches (art_trace.hip).
//
//   k_raygen / k_shade_compact / k_resolve_last / k_fold / k_fold_level / k_accumulate / k_accumulate_moments / k_debug   the stages over
//                  compacted work sets (per-item functions in art_shade.h); k_shade / k_finish: the plain in-place schedule;
//                  k_bump / k_acc_items: the counters of a batch.
//
// Replaces PathTrace (ray_tracer-integrators.adb:82-301) and the DoPass pixel loop (integrators.adb:25-71).  The diagnostic builds
// -DART_LANE_PROBE and -DART_TIME_PROBE (art_isect.h; profiles/lane_probe.py, profiles/time_probe.py) study k_shade_compact: a
// __device__ variable exists once per translation unit, so the reader of g_lane_probe, art_debug_lane_probe, is at the end of this file.
#include <hip/hip_runtime.h>
#include "art_stages.h"
#include "art_kernel_common.h"
#include "art_shade.h"
#include "art_camera_order.h"

namespace art {

// ------------------------------------------------------------------------------------------------
// wavefront stages
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_raygen(const DevFrame F, const DevScene S, const DevPaths Q) {
  __shared__ DevSphere s_sph[kAnalyticLdsSpheres];
  __shared__ DevLight s_lgt[kAnalyticLdsLights];
  StageCtx cx;
  if (Q.rec != nullptr && S.n_spheres <= kAnalyticLdsSpheres && S.n_lights <= kAnalyticLdsLights) {      // record mode: the camera ray's analytic intersection happens here
    if ((int)threadIdx.x < S.n_spheres) s_sph[threadIdx.x] = S.spheres[threadIdx.x];
    if ((int)threadIdx.x < S.n_lights) s_lgt[threadIdx.x] = S.lights[threadIdx.x];
    __syncthreads();
    cx.lds_spheres = as_lds(&s_sph[0]); cx.lds_lights = as_lds(&s_lgt[0]);
  }
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  // record mode: a wave's 64 records are 4 KB of consecutive bytes; staged through LDS so that every store instruction writes one
  // contiguous kilobyte (as in k_shade_compact)
  constexpr int kPitch = 64 + 1;
  __shared__ Rec4 s_stage[4][4 * kPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool staged = (Q.rec != nullptr) && Q.has_bvh;
  if (staged) { cx.stage = s_stage[wave]; cx.stage_pitch = kPitch; cx.stage_item = lane; }
  cx.hot_layout = (Q.hot != nullptr);                    // record schedule: the hit record goes out through the bank's block, as a streaming store
  if (slot < Q.P) raygen_slot(F, S, Q, slot, cx);
  if (staged) {
    wave_lds_sync();
    const int first = slot - lane;
    const int n_pieces = 4 * max(0, min(64, Q.P - first));
    Rec4* out = Q.rec + 4 * (size_t)first;
    for (int pc = lane; pc < n_pieces; pc += 64) put_s(out, pc, s_stage[wave][(pc & 3) * kPitch + (pc >> 2)]);      // (read once, by the trace kernel: non-temporal)
  }
}

__global__ __launch_bounds__(256) void k_shade(const DevFrame F, const DevScene S, const DevPaths Q, int bounce) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot < Q.P) shade_slot(F, S, Q, slot, bounce);
}

// ------------------------------------------------------------------------------------------------
// k_shade_compact: one bounce over a compacted work set.  Every stage reads the items of the paths that still need something (input
// set `Qi`: rays, hits, per-path state, item -> slot map) and writes only the items that will need something at the next stage to the
// output set `Qo`, densely: the kernels that follow (the trace kernel's record fetch, the next shade) then stream full 128-byte lines
// of live data instead of lines in which a quarter of the slots is alive.
//
// A workgroup handles a chunk of 256 x PER items in three steps (round 4):
//   1. classify: every item's class (item_class: its surface material, or CLS_CHEAP when the path ends at this hit), from the flags, the
//      hit key and the material type alone; per class, a wave reserves its items' places in the class with ONE LDS atomic (ballot +
//      prefix inside the wave);
//   2. sort: the chunk's items are laid out class by class in LDS (s_perm), surface classes first -- they are the survivors: ONE global
//      atomic reserves their range of the output set, item r of the sorted chunk goes to output item base + r;
//   3. shade in sorted order: thread t takes sorted items t, t + 256, ...: a wave's 64 items are consecutive in the sorted chunk, so
//      they are of ONE class except where two classes meet.  Before the sort a wave ran every material present in it with that material's
//      lanes only: 31 of 64 lanes enabled per VALU instruction (C3, C4), 27 (C5), e.g. on C4 71 % of the waves walked the Phong code
//      (four binary64 pow) for three lanes on the back wall (profiles/r4_shade/lane_probe_*.txt).
// The survivors of a wave's round are consecutive output items: their trace records are one contiguous piece of the output bank, the
// extension rays first, then the shadow rays (REC_BOTH).  The wave builds the records of one kind (make_record: analytic primitives
// intersected = the starting bound, slab set-up), stages them in LDS and copies them out 16 bytes per lane to consecutive addresses.
// That copy-out sits inside shade_item's emit_ray: every kept item of a wave is a surface item and takes the surface branch together,
// which rests on the compiler keeping ONE call site for it; it is therefore checked at run time -- every record copied must name the hit
// slot its position implies, else the stage counts a lost path, and a lost path fails art_synchronize.  (Copying out at
// a point every lane of the wave reaches costs 30 more VGPRs: DESIGN_HISTORY.md, the ADVICE (low) staged copy-out row.)
// ------------------------------------------------------------------------------------------------
// items per workgroup = 256 x kShadePerThread, one global atomic per workgroup.  4 per thread, not 16: a thread's items one after the
// other are its critical path (round 3, DESIGN_HISTORY.md; profiles/r4_shade/ab_waves_per_thread_sweep.txt).
constexpr int kShadePerThread = 4;
// 6 waves per SIMD (80 VGPRs): left to itself the compiler takes 111 VGPRs = 4 waves, slower (round 3; 5 / 7 waves: profiles/r5_shade/ab17_stage_waves_final_kernel.txt)
constexpr int kShadeWavesPerSimd = 6;
// CAMERA: bounce 0 over raygen's bank (DevPaths::synth0: flags, previous pdf and the camera ray are recomputed, not read) -- its own
// instantiation, so that the other bounces' code is exactly what it was (as one kernel the extra branch cost 17 more spilled VGPRs: +7 %)
// CAMERA items are slots, so a round may take ANY 256 consecutive slots of a sample row: with option camera_order = 1 round k of
// workgroup g takes unit g * PER + k of the tile-major order of art_camera_order.h (all samples of 1024 pixels before the next 1024)
// instead of slots [c0 + 256 k, c0 + 256 k + 256).  The unit's first slot and size are wave-uniform: scalars, computed once per round.
// The stage's arguments as ONE struct: about 240 dwords of scene header and array pointers.  Taken by value the compiler loads all of them
// into SGPRs at the kernel's entry and keeps them live to its end (spilled to VGPR lanes).  The code reads the fields through a pointer
// to the kernarg segment instead, laundered at the head of every round so that a field is a scalar load (scalar cache) where it is used
// (profiles/r4_shade/ab_kernarg.txt).
struct ShadeKernArgs {
  DevFrame F; DevScene S; DevPaths Qi; DevPaths Qo; int bounce;
  const int* n_in_ptr; int* n_out_ptr; uint32_t* slot_out; unsigned long long* lost; unsigned long long* rays_a; unsigned long long* rays_b;
  int cam_order, cam_sn;      // CAMERA only (the last fields: the other instantiation's offsets are what they were): option camera_order, samples of the batch (P / npix)
};
static_assert(sizeof(ShadeKernArgs) <= 4096 && __is_trivially_copyable(ShadeKernArgs), "ShadeKernArgs is the kernel's ONLY parameter: it sits at offset 0 of the kernarg segment");
typedef const __attribute__((address_space(4))) ShadeKernArgs* ShadeKArgs;
__device__ __forceinline__ ShadeKArgs launder_kargs(ShadeKArgs k) { unsigned long long r = (unsigned long long)k; asm volatile("" : "+s"(r)); return (ShadeKArgs)r; }

template <int PER, bool CAMERA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kShadeWavesPerSimd))) void k_shade_compact(const ShadeKernArgs A_by_value) {
  ShadeKArgs K = launder_kargs((ShadeKArgs)__builtin_amdgcn_kernarg_segment_ptr());
  const DevFrame& F = *(const DevFrame*)&K->F; const DevScene& S = *(const DevScene*)&K->S; const DevPaths& Qi = *(const DevPaths*)&K->Qi; const DevPaths& Qo = *(const DevPaths*)&K->Qo;
  const int bounce_arg = K->bounce;
  const int* const n_in_ptr = K->n_in_ptr; int* const n_out_ptr = K->n_out_ptr;
  unsigned long long* const rays_a = K->rays_a; unsigned long long* const rays_b = K->rays_b;
  const int bounce = CAMERA ? 0 : bounce_arg;            // (a literal for the camera instantiation: no shadow test can be owed, nothing is pending)
  constexpr int kShadeChunk = 256 * PER;
  __shared__ int s_tot[PER * kItemClasses];                // items of each class in each round (256 items) of the chunk
  __shared__ int s_base, s_rays;
  __shared__ int s_nall[PER], s_nkeep[PER], s_out0[PER];   // per round: items, survivors, first output item (relative to s_base)
  __shared__ int s_slot0[CAMERA ? PER : 1];                // CAMERA: per round, the first of its 256 consecutive slots
  // [round][sorted position] -> { hit key, thread that classified the item | surface flag << 8 | material index << 9 }: what the
  // classification fetched goes along (ItemHint), so that shade_item asks for the triangle's normals and the material record at once
  __shared__ uint2 s_hint[kShadeChunk];
  // a wave's trace records of one kind, [quarter][record] (+1: four consecutive records' quarters fall into four banks)
  constexpr int kStagePitch = 64 + 1;
  __shared__ Rec4 s_stage[4][4 * kStagePitch];
  constexpr int kShadeLdsLights = 8;                    // (8, not k_analytic's 16: with the hints the workgroup's LDS must stay below 160 KB / 6)
  __shared__ DevSphere s_sph[kAnalyticLdsSpheres];      // the scene's spheres and lights, fetched once per workgroup (every emitted ray is tested against them)
  __shared__ DevLight s_lgt[kShadeLdsLights];
  const int n_in = n_in_ptr ? *n_in_ptr : Qi.P;
  const int c0 = blockIdx.x * kShadeChunk;
  const int cam_order = CAMERA ? K->cam_order : 0;
  if (CAMERA && cam_order) { if ((int)blockIdx.x * PER >= camera_order_units(Qi.npix, K->cam_sn)) return; }      // the grid covers the visiting space, in units
  else if (c0 >= n_in) return;                           // the grid covers Qi.P items; the work set has shrunk to n_in
  // (the material table stays in global memory: a 40-byte per-lane-indexed record out of LDS measured 7 % slower than the cached global read)
  const bool tables_in_lds = (S.n_spheres <= kAnalyticLdsSpheres) && (S.n_lights <= kShadeLdsLights);
  if (tables_in_lds) {
    if ((int)threadIdx.x < S.n_spheres) s_sph[threadIdx.x] = S.spheres[threadIdx.x];
    if ((int)threadIdx.x < S.n_lights) s_lgt[threadIdx.x] = S.lights[threadIdx.x];
  }
  if (threadIdx.x < PER * kItemClasses) s_tot[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_rays = 0;
  __syncthreads();
  StageCtx tables;
  tables.hot_layout = true;
  if (tables_in_lds) { tables.lds_spheres = as_lds(&s_sph[0]); tables.lds_lights = as_lds(&s_lgt[0]); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lanes_below = (1ull << lane) - 1ull;
#if defined(ART_TIME_PROBE)
  __shared__ unsigned long long s_tprobe[4][2];        // per wave: { time of the previous probe, address of the workgroup's table }
  __shared__ unsigned long long s_tacc[2 * 32];
  if (threadIdx.x < 64) s_tacc[threadIdx.x] = 0;
  if (lane == 0) { s_tprobe[wave][0] = __builtin_readcyclecounter(); s_tprobe[wave][1] = (unsigned long long)(uintptr_t)s_tacc; }
  __syncthreads();
  tables.tprobe = &s_tprobe[wave][0];
#endif
  // ---- 1. classify; a wave's items of one class take consecutive places in the class (of their round)
  int cls[PER], rank[PER]; ItemHint hint[PER];
  {
    // the PER classifications as ONE batch of loads per step (item_classes: 3 memory round trips; item by item through item_class they were 20)
    int wk[PER]; bool on[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (CAMERA) {
        OrderUnit u; u.slot0 = c0 + k * 256; u.count = n_in - u.slot0;      // slot order
        if (cam_order) {
          const int ui = (int)blockIdx.x * PER + k;                          // tile-major: a unit past the last one is padding
          u.count = 0;
          if (ui < camera_order_units(Qi.npix, K->cam_sn)) u = camera_order_unit(Qi.npix, K->cam_sn, ui);
        }
        u.slot0 = __builtin_amdgcn_readfirstlane(u.slot0); u.count = __builtin_amdgcn_readfirstlane(u.count);
        wk[k] = u.slot0 + (int)threadIdx.x; on[k] = (int)threadIdx.x < u.count;
        if (threadIdx.x == 0) s_slot0[k] = u.slot0;                          // (read after barrier 1)
      } else { wk[k] = c0 + k * 256 + (int)threadIdx.x; on[k] = wk[k] < n_in; }
      hint[k].key = KEY_MISS; hint[k].mat = 0; cls[k] = kItemClasses;
    }
    item_classes<PER>(S, Qi, wk, on, tables, CAMERA, cls, hint);
  }
  ART_TPROBE(tables.tprobe, 64);      // classification loads
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int c = cls[k];
    const bool surface = c < CLS_CHEAP;
    hint[k].mat = (int32_t)(threadIdx.x | (surface ? 256u : 0u) | ((uint32_t)hint[k].mat << 9));
    rank[k] = 0;
#pragma unroll
    for (int q = 0; q < kItemClasses; ++q) {
      const uint64_t m = __builtin_amdgcn_ballot_w64(c == q);
      if (m != 0) {                                        // wave-uniform
        int b = 0;
        if (lane == 0) b = atomicAdd(&s_tot[k * kItemClasses + q], (int)__popcll(m));
        b = __builtin_amdgcn_readfirstlane(b);
        if (c == q) rank[k] = b + (int)__popcll(m & lanes_below);
      }
    }
  }
  ART_TPROBE(tables.tprobe, 65);      // class ranks (ballots + LDS atomics)
  __syncthreads();
  ART_TPROBE(tables.tprobe, 66);      // barrier 1
  // ---- 2. sort every round: class q starts where the classes before it end; the surface classes (the survivors) come first.
  // The sort stays inside a round's 256 items: the four waves of the workgroup then read one 1-KB window of every array at the same time
  // (sorted over the whole chunk, a wave's loads touched lines whose other halves were fetched again three rounds later: +43 % bytes
  // fetched, +22 % written back, 16-27 % slower although it ran 29 % fewer VALU instructions -- profiles/r4_shade/ab_sort_chunk.txt)
  const bool keeps = stage_keeps_surfaces(F, bounce);
  int total_keep = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    int st = 0, mine = 0, nkeep = 0;
#pragma unroll
    for (int q = 0; q < kItemClasses; ++q) {
      if (q == CLS_CHEAP) nkeep = keeps ? st : 0;
      mine = (cls[k] == q) ? st : mine;
      st += s_tot[k * kItemClasses + q];
    }
    if (threadIdx.x == 0) { s_nall[k] = st; s_nkeep[k] = nkeep; s_out0[k] = total_keep; }
    total_keep += nkeep;
    if (cls[k] < kItemClasses) s_hint[k * 256 + mine + rank[k]] = make_uint2(hint[k].key, (uint32_t)hint[k].mat);
  }
  if (threadIdx.x == 0) s_base = total_keep ? atomicAdd(n_out_ptr, total_keep) : 0;
  __syncthreads();
  const int base = s_base;
  ART_TPROBE(tables.tprobe, 67);      // sort, output reservation (global atomic), barrier 2
  // ---- 3. shade in sorted order
  const bool staged = (Qo.rec != nullptr) && Qo.has_bvh;
  int n_rays = 0;
#pragma unroll 1
  for (int k = 0; k < PER; ++k) {
    const ShadeKArgs K2 = launder_kargs(K);               // the round's own view of the arguments: nothing loaded before survives in a register
    const DevFrame& F = *(const DevFrame*)&K2->F; const DevScene& S = *(const DevScene*)&K2->S; const DevPaths& Qi = *(const DevPaths*)&K2->Qi; const DevPaths& Qo = *(const DevPaths*)&K2->Qo;
    unsigned long long* const lost = K2->lost;            // (the output items' slot words are written by shade_item: Qo's HF_SLOT field IS K->slot_out)
    ART_TPROBE(tables.tprobe, 70);    // round bookkeeping (and, after the first round, whatever followed the last probe of the item before)
    // Wave w takes the sorted positions [64 w, 64 w + 64) of every round (rotating the tiles over the waves gained nothing:
    // profiles/r5_shade/ab8_rotate.txt).
    const int r = wave * 64 + lane;                       // position in the sorted round
    const int n_all_k = s_nall[k], n_keep_k = s_nkeep[k], out0_k = s_out0[k];
    const int wo = r < n_keep_k ? base + out0_k + r : -1;
    if (r < n_all_k) {
      const uint2 hk = s_hint[k * 256 + r];
      const int w = (CAMERA ? __builtin_amdgcn_readfirstlane(s_slot0[k]) : c0 + k * 256) + (int)(hk.y & 255u);
      ItemHint ih; ih.key = hk.x; ih.mat = (hk.y & 256u) ? (int32_t)(hk.y >> 9) : -1;      // mat < 0: no hint (shade_item)
      // (the output item's slot word is written by shade_item with the item's other words: qo.slot_id IS slot_out)
      StageCtx cy = tables;
      if (staged) {
        const int nk = min(64, max(0, n_keep_k - wave * 64)), per = (Qo.rec_mode == REC_BOTH) ? 2 : 1;
        const size_t first = (size_t)per * (size_t)(base + out0_k + wave * 64);
        cy.stage = s_stage[wave]; cy.stage_pitch = kStagePitch; cy.stage_item = lane; cy.stage_count = nk; cy.lost = lost;
        cy.rec_base[0] = first; cy.rec_base[1] = (per == 2) ? first + (size_t)nk : first;
      }
      n_rays += shade_item(F, S, Qi, Qo, w, wo, bounce, lost, cy, &ih, CAMERA ? 1 : 0, 1);
    }
  }
  ART_TPROBE(tables.tprobe, 68);      // end of the last round
#if defined(ART_TIME_PROBE)
  __syncthreads();
  if (threadIdx.x < 64 && s_tacc[threadIdx.x] != 0) atomicAdd(&g_lane_probe[2 * 64 + threadIdx.x], s_tacc[threadIdx.x]);
#endif
  // record mode: the rays just emitted are the closest-hit queries of the next trace launch (k_analytic counts them in the plain layout)
  if (Qo.rec != nullptr && rays_a != nullptr) {
    for (int off = 32; off > 0; off >>= 1) n_rays += __shfl_xor(n_rays, off);
    if (lane == 0 && n_rays) atomicAdd(&s_rays, n_rays);
    __syncthreads();
    if (threadIdx.x == 0 && s_rays) { atomicAdd(rays_a, (unsigned long long)s_rays); if (rays_b) atomicAdd(rays_b, (unsigned long long)s_rays); }
  }
}

__global__ void k_bump(unsigned long long* a, unsigned long long* b, unsigned long long n) { *a += n; if (b) *b += n; }
__global__ void k_acc_items(const int* live, int depth, int P, unsigned long long* items) {
  unsigned long long in = (unsigned long long)P;
  for (int b = 0; b < depth && b < 16; ++b) { const unsigned long long out = (unsigned long long)live[32 * (b + 1)]; items[b] += in; items[16 + b] += out; in = out; }
}

// the shadow tests still owed after the last trace, over the last work set; then the fold over all slots
__global__ __launch_bounds__(256) void k_resolve_last(const DevPaths Q, const int* __restrict__ n_ptr, int last_level) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < *n_ptr) resolve_last_shadow(Q, w, last_level);
}
__global__ __launch_bounds__(256) void k_fold(const DevFrame F, const DevPaths Q) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot < Q.P) fold_slot(F, Q, slot);
}

// dense fold records: one level (art_shade.h fold_level_item).  n_ptr: the level's item count (nullptr: all Q.P slots = level 0)
__global__ __launch_bounds__(256) void k_fold_level(const DevFrame F, const DevPaths Q, int level, int deepest, const int* __restrict__ n_ptr,
                                                    const float* __restrict__ nxt_r, const float* __restrict__ nxt_g, const float* __restrict__ nxt_b,
                                                    float* __restrict__ cur_r, float* __restrict__ cur_g, float* __restrict__ cur_b) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = n_ptr ? *n_ptr : Q.P;
  if (w < n) fold_level_item(F, Q, level, w, deepest != 0, nxt_r, nxt_g, nxt_b, cur_r, cur_g, cur_b);
}

__global__ __launch_bounds__(256) void k_finish(const DevFrame F, const DevPaths Q, int last_level) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot < Q.P) finish_slot(F, Q, slot, last_level);
}

__global__ __launch_bounds__(256) void k_accumulate(const DevFrame F, const DevPaths Q, int samples_in_batch, float* accum) {
  const int pl = blockIdx.x * blockDim.x + threadIdx.x;
  if (pl < Q.npix) accumulate_pixel(F, Q, pl, samples_in_batch, accum);
}

// the same walk with the luminance moments of art_bind_moments next to the accum (launched instead of k_accumulate while moments are bound)
__global__ __launch_bounds__(256) void k_accumulate_moments(const DevFrame F, const DevPaths Q, int samples_in_batch, float* accum, float* moments) {
  const int pl = blockIdx.x * blockDim.x + threadIdx.x;
  if (pl < Q.npix) accumulate_pixel_moments(F, Q, pl, samples_in_batch, accum, moments);
}

// Debug_Ray_Tracing (ray_tracer.adb:208-238): palette colour of the primary hit's matId, plus raw ids
__global__ __launch_bounds__(256) void k_debug(const DevFrame F, const DevScene S, const DevPaths Q, float* accum,
                                               int32_t* prim_index, int32_t* mat_id, int32_t* prim_type) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= Q.P) return;
  uint32_t pixel, sample;
  slot_to_sample(Q, slot, pixel, sample);
  const DevHit hq = Q.hit[slot];
  const uint32_t key = hq.key;
  f3 col = mk3(0.0f, 0.0f, 0.0f);
  int32_t pi = -1, mi = -1, pt = -1;
  if (key != KEY_MISS) {
    const f3 o = mk3(Q.ray_ox[slot], Q.ray_oy[slot], Q.ray_oz[slot]), d = mk3(Q.ray_dx[slot], Q.ray_dy[slot], Q.ray_dz[slot]);
    const Surface sf = surface_at(S, o, d, hq.t, key, hq.u, hq.v);
    col = debug_palette(sf.mat_id);
    mi = sf.mat_id; pi = (int32_t)(key & KEY_INDEX_MASK);
    const uint32_t cls = key & ~KEY_INDEX_MASK;   // geometry.ads:55 Primitive'Pos: plane 0, sphere 1, triangle 2, quad 3
    pt = (cls == KEY_CORNELL) ? 0 : (cls == KEY_SPHERE) ? 1 : (cls == KEY_QUAD) ? 3 : 2;
  }
  accum[3 * (size_t)pixel] = col.x; accum[3 * (size_t)pixel + 1] = col.y; accum[3 * (size_t)pixel + 2] = col.z;
  if (prim_index) prim_index[pixel] = pi;
  if (mat_id) mat_id[pixel] = mi;
  if (prim_type) prim_type[pixel] = pt;
}

// ------------------------------------------------------------------------------------------------
// launchers (the only symbols art_api.cpp needs from this translation unit)
// ------------------------------------------------------------------------------------------------
void launch_raygen(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q) {
  hipLaunchKernelGGL(k_raygen, dim3(blocks_for(Q.P)), dim3(256), 0, st, F, S, Q);
}
void launch_shade(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q, int bounce) {
  hipLaunchKernelGGL(k_shade, dim3(blocks_for(Q.P)), dim3(256), 0, st, F, S, Q, bounce);
}
#if defined(ART_LANE_PROBE)
__global__ void k_probe_on(int v) { g_lane_probe_on = v; }
#endif
void launch_shade_compact(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Qi, const DevPaths& Qo, int bounce,
                          const int* n_in, int* n_out, uint32_t* slot_out, unsigned long long* lost, unsigned long long* rays_a, unsigned long long* rays_b,
                          int per, int camera_order) {
  const bool camera = Qi.synth0 && Qi.slot_id == nullptr;
  const int per_now = (per == 2) ? 2 : kShadePerThread;      // items per thread of this launch
  // rounds of 256 items: the items of the bank, or (bounce 0, option camera_order) the units of the tile-major visiting order
  const int cam_sn = Qi.npix > 0 ? Qi.P / Qi.npix : 0;
  const bool tile_major = camera && camera_order != 0 && cam_sn > 0;
  const int rounds = tile_major ? camera_order_units(Qi.npix, cam_sn) : (Qi.P + 255) / 256;
  const dim3 grid((rounds + per_now - 1) / per_now);
#if defined(ART_LANE_PROBE)
  hipLaunchKernelGGL(k_probe_on, dim3(1), dim3(1), 0, st, 1);
#endif
  ShadeKernArgs A; A.F = F; A.S = S; A.Qi = Qi; A.Qo = Qo; A.bounce = bounce; A.n_in_ptr = n_in; A.n_out_ptr = n_out; A.slot_out = slot_out; A.lost = lost; A.rays_a = rays_a; A.rays_b = rays_b;
  A.cam_order = tile_major ? 1 : 0; A.cam_sn = cam_sn;
  with_flags(per_now == 2, camera, [&](auto TWO, auto CAMERA) {
    hipLaunchKernelGGL((k_shade_compact<decltype(TWO)::value ? 2 : kShadePerThread, decltype(CAMERA)::value>), grid, dim3(256), 0, st, A);
  });
#if defined(ART_LANE_PROBE)
  hipLaunchKernelGGL(k_probe_on, dim3(1), dim3(1), 0, st, 0);
#endif
}
void launch_acc_items(hipStream_t st, const int* live, int depth, int P, unsigned long long* items) { hipLaunchKernelGGL(k_acc_items, dim3(1), dim3(1), 0, st, live, depth, P, items); }
void launch_bump(hipStream_t st, unsigned long long* a, unsigned long long* b, unsigned long long n) { hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, st, a, b, n); }
void launch_resolve_last(hipStream_t st, const DevPaths& Q, const int* n, int last_level) {
  hipLaunchKernelGGL(k_resolve_last, dim3(blocks_for(Q.P)), dim3(256), 0, st, Q, n, last_level);
}
void launch_fold(hipStream_t st, const DevFrame& F, const DevPaths& Q) {
  hipLaunchKernelGGL(k_fold, dim3(blocks_for(Q.P)), dim3(256), 0, st, F, Q);
}
// the whole fold over dense records: levels max_depth - 1 .. 0, ping-pong between the term arrays (odd levels) and rad (even levels: level 0
// ends in rad, where k_accumulate reads).  counts[32 * k] = item count of level k (k >= 1)
void launch_fold_levels(hipStream_t st, const DevFrame& F, const DevPaths& Q, int max_depth, const int* counts) {
  for (int k = max_depth - 1; k >= 0; --k) {
    float* cur[3] = {(k & 1) ? Q.term_r : Q.rad_r, (k & 1) ? Q.term_g : Q.rad_g, (k & 1) ? Q.term_b : Q.rad_b};
    const float* nxt[3] = {(k & 1) ? Q.rad_r : Q.term_r, (k & 1) ? Q.rad_g : Q.term_g, (k & 1) ? Q.rad_b : Q.term_b};
    hipLaunchKernelGGL(k_fold_level, dim3(blocks_for(Q.P)), dim3(256), 0, st, F, Q, k, k == max_depth - 1 ? 1 : 0, k == 0 ? nullptr : counts + 32 * k,
                       nxt[0], nxt[1], nxt[2], cur[0], cur[1], cur[2]);
  }
}
void launch_finish(hipStream_t st, const DevFrame& F, const DevPaths& Q, int last_level) {
  hipLaunchKernelGGL(k_finish, dim3(blocks_for(Q.P)), dim3(256), 0, st, F, Q, last_level);
}
void launch_accumulate(hipStream_t st, const DevFrame& F, const DevPaths& Q, int samples_in_batch, float* accum) {
  hipLaunchKernelGGL(k_accumulate, dim3(blocks_for(Q.npix)), dim3(256), 0, st, F, Q, samples_in_batch, accum);
}
void launch_accumulate_moments(hipStream_t st, const DevFrame& F, const DevPaths& Q, int samples_in_batch, float* accum, float* moments) {
  hipLaunchKernelGGL(k_accumulate_moments, dim3(blocks_for(Q.npix)), dim3(256), 0, st, F, Q, samples_in_batch, accum, moments);
}
void launch_debug(hipStream_t st, const DevFrame& F, const DevScene& S, const DevPaths& Q, float* accum, int32_t* prim_index, int32_t* mat_id, int32_t* prim_type) {
  hipLaunchKernelGGL(k_debug, dim3(blocks_for(Q.P)), dim3(256), 0, st, F, S, Q, accum, prim_index, mat_id, prim_type);
}

}  // namespace art

#if defined(ART_LANE_PROBE)
// diagnostic build: read (and clear) the lane probes of art_isect.h
extern "C" int art_debug_lane_probe(unsigned long long* out, int n) {
  unsigned long long z[2 * 96] = {};
  if (n > 2 * 96) n = 2 * 96;
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lane_probe), (size_t)n * 8) != hipSuccess) return 1;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_lane_probe), z, sizeof z) != hipSuccess;
}
#endif
