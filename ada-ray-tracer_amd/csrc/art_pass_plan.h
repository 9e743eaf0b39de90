// art_pass_plan.h -- the two pieces of pure host logic of a render pass (art_render.cpp): the shape of its batches and the shade stage's
// items-per-thread trial.  Plain C++17, no HIP: tests/pass_plan_host compiles it with g++ (tests/test_pass_plan_host.py).
#pragma once
#include <algorithm>
#include <cstdint>

namespace art {

// A batch = pixel chunk x sample chunk with pc * sc <= max(cap, per) path slots.  npix >= 1 pixels, S >= 1 samples this pass (a multiple
// of per), per = 4 with anti-aliasing on (a Generate4RayDirections group), else 1; cap = option batch_paths, or what is left of it after the
// caller halved it for want of memory.
struct BatchPlan { int pc, sc; };
inline BatchPlan plan_batch(int npix, int S, int per, int64_t cap) {
  cap = std::max<int64_t>(cap, per);
  BatchPlan b;
  // Samples first needs room for all S samples of at least kMinPixelChunk pixels (or of the whole frame); with less, the shape is the
  // pixels-first one of before.  The minimum is a compatibility rule, not a measured one: tests/test_gpu_camera_dedup.py
  // (test_small_batches) pins the pixels-first plan at the smallest batch_paths (1024 paths, 8 samples: 256 pixels x 4 samples with
  // AA on, 8 * W * H camera rays traced), where the plain rule "sc = S whenever batch_paths >= S" gives 128 pixels x 8 samples.  256 is
  // that pinned pixel chunk.  Smaller chunks work (a last partial chunk is samples first at any size); nothing below 256 * S paths
  // per batch has been timed either way.
  constexpr int64_t kMinPixelChunk = 256;
  if (cap / S >= std::min<int64_t>(npix, kMinPixelChunk)) {
    // Samples first: a pixel chunk carries all S samples of the pass, so each distinct camera ray of the pass is generated and traced in
    // exactly one batch (camera_dedup: U * pn rays per batch, U * npix per pass, however many pixel chunks there are).  The pixel map is
    // dealt in 32 x 32 tiles: a chunk that does not cover the frame is a whole number of them.
    b.sc = S;
    b.pc = (int)std::min<int64_t>(npix, std::max<int64_t>(1, cap / b.sc));
    if (b.pc < npix && b.pc >= 1024) b.pc = b.pc / 1024 * 1024;
  } else {
    // too few path slots for 256 pixels with all their samples: pixels first, as many Generate4RayDirections groups per pixel as fit; the camera
    // rays of a pixel chunk are then traced once per sample chunk
    b.pc = (int)std::min<int64_t>(npix, std::max<int64_t>(1, cap / per));
    b.sc = (int)std::min<int64_t>(S, std::max<int64_t>(per, (cap / b.pc) / per * per));
  }
  return b;
}

// The items-per-thread trial of the shade stage (art_api_internal.h Options::opt_shade_per), per context.  Nothing in it waits for the
// GPU: next() says what a batch runs with and whether its shade launches' event pairs carry a trial's tag, add() takes the times of the
// pairs a synchronise reads, decide() keeps the faster setting once both trials are in.
struct ShadeTrial {
  int per = 0, phase = 0;        // phase: 0 warm batch next, 1 trial A (4) next, 2 trial B (2) next, 3 both enqueued, 4 decided (per)
  double ms[2] = {0.0, 0.0}; int64_t P[2] = {0, 0}; int redo = 0;
  unsigned gen = 0;              // a trial's event pairs carry its generation (mod 4); a reset or a re-done trial starts a new one

  // a new scene, another frame or batch size: measure again
  void reset() { phase = 0; redo = 0; gen += 1; }

  struct Batch { int trial, shade_per; };      // trial: 0 none, 1 / 2 = the batch is trial A / B
  // the batch of `paths` paths that is enqueued next.  pinned_option: Options::opt_shade_per (0: measured); record_schedule: only the
  // compacted schedule has the stage
  Batch next(int64_t paths, int pinned_option, bool record_schedule) {
    Batch b = {0, pinned_option ? pinned_option : (phase >= 4 ? per : 4)};
    if (pinned_option == 0 && phase < 3 && record_schedule) {
      if (phase == 0) phase = 1;                                          // the warm batch: 4 items per thread, not measured
      else if (phase == 1) { b.trial = 1; ms[0] = 0.0; P[0] = paths; phase = 2; }
      else if (paths == P[0]) { b.trial = 2; b.shade_per = 2; ms[1] = 0.0; P[1] = paths; phase = 3; }
      else if (++redo > 3) { per = 4; phase = 4; }                        // batch sizes keep changing: no trial, 4 items per thread
      else { b.trial = 1; gen += 1; ms[0] = 0.0; P[0] = paths; }          // a batch of another size: trial A again, on this size (new generation: the old trial's events no longer count)
    }
    return b;
  }
  // the time of one shade launch of trial 1 / 2 whose tag carried generation g (two bits of it): another generation's no longer counts
  void add(int trial, unsigned g, double t) { if ((trial == 1 || trial == 2) && (g & 3) == (gen & 3)) ms[trial - 1] += t; }
  // both trial batches are done (the caller's stream is idle): keep the faster setting from here on.  true: decided by this call
  bool decide() {
    if (phase != 3) return false;
    per = (ms[1] < ms[0]) ? 2 : 4;
    phase = 4;
    return true;
  }

  // The tag of an event pair of Ctx::stage_pairs: kind (0 trace kernel, 1 shade stage, 2 raygen, 3 fold group) | trial << 4 | the trial's
  // generation (mod 4) << 6; a pair outside a trial carries no generation.
  struct Tag { int kind, trial; unsigned gen; };
  static uint8_t encode(int kind, int trial, unsigned g) { return (uint8_t)(kind | (trial << 4) | (trial ? (g & 3) << 6 : 0)); }
  static Tag decode(uint8_t tag) { return {tag & 15, (tag >> 4) & 3, (unsigned)(tag >> 6)}; }
  uint8_t tag(int kind, int trial = 0) const { return encode(kind, trial, gen); }
};

}  // namespace art
