"""GPU time of art_temporal_device and of art_set_camera, measured once on one MI355X.

Workload: C4 (scenes.synthetic_scene(1000000, 4)) at 1920 x 1080, accum and moments bound, one PT_MIS pass of 4 spp without
anti-aliasing per frame, feature buffers of the frame.
  (a) art_temporal_device against art_denoise_svgf_device on the same frame, in one process, alternating, torch events around each call
      (the previous history is that of a camera 0.05 to the right: a real reprojection); mean and spread over --reps calls after a warm-up.
  (b) floor_ms: the temporal call's compulsory 156 B per pixel at the 6.3 TB/s profiles/denoise/ measured.
  (c) art_set_camera + one pass against art_upload_scene + one pass, host clock around call + pass + synchronise.
  (d) ArtStageStats of one pass on a fresh viewport at the uploaded camera, before any new call and after set_camera away and back,
      re-uploads and temporal calls: the same launches, batches and items.

usage: python profiles/temporal/measure.py [--out profiles/temporal/measure.json] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H, SPP = 1920, 1080, 4
BANDWIDTH_TBS = 6.3          # profiles/denoise/README.md
BYTES_PER_PIXEL = 156        # csrc/art_temporal.hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "measure.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    sd = scenes.synthetic_scene(1000000, 4)
    cams = [(np.array([0.05 * k, 2.55, 12.5], np.float32), np.eye(4, dtype=np.float32)) for k in range(2)]
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    p = art.Backend.pass_params(art.PT_MIS, False, 8, SPP, seed=7)

    def stage_counts():
        st = be.stage_stats()
        return [int(st.shade_launches), int(st.batches)] + [int(v) for v in st.items_in] + [int(v) for v in st.items_out]

    def frame():
        be.resize(W, H)
        spp = be.render_pass_device(p, 0)
        be.synchronize()
        return spp

    be.upload_scene(sd)
    be.bind_accum(accum); be.bind_moments(moments)
    frame()
    stages_before = stage_counts()
    be.set_camera(*cams[1]); frame()
    aovs = be.render_aovs_torch(p, want=("albedo", "normal", "depth", "prim_index"))
    cur = dict(aovs, color=accum, moments=moments)
    hist = be.temporal_torch(cur, None, cams[1], None, SPP, scale=1.0 / SPP)[3]
    # (c) the camera: setter + pass against upload + pass
    t_set, t_up = [], []
    for k in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        be.set_camera(*cams[(k + 1) % 2]); frame()
        t_set.append((time.perf_counter() - t0) * 1e3)
    for k in range(3):
        for j in range(3):
            sd.desc.cam_pos[j] = float(cams[k % 2][0][j])
        torch.cuda.synchronize(); t0 = time.perf_counter()
        be.upload_scene(sd); be.bind_accum(accum); be.bind_moments(moments); frame()
        t_up.append((time.perf_counter() - t0) * 1e3)
    be.set_camera(*cams[0]); frame()             # the first frame's camera again: the same pass as stages_before counted
    stages_after = stage_counts()
    aovs = be.render_aovs_torch(p, want=("albedo", "normal", "depth", "prim_index"))
    cur = dict(aovs, color=accum, moments=moments)
    # (a) alternating
    times = {"temporal": [], "svgf": []}
    found = None
    for r in range(args.reps + 3):
        for name in ("temporal", "svgf"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if name == "temporal":
                found = be.temporal_torch(cur, hist, cams[0], cams[1], SPP, scale=1.0 / SPP)[2]
            else:
                be.denoise_svgf_torch(accum, moments, SPP, albedo=aovs["albedo"], normal=aovs["normal"], depth=aovs["depth"], scale=1.0 / SPP)
            e1.record(); e1.synchronize()
            if r >= 3:
                times[name].append(e0.elapsed_time(e1))
    res = {"what": "C4 at %d x %d, %d spp per frame; one MI355X; GPU ms per call (torch events), %d calls each, alternating" % (W, H, SPP, args.reps),
           "temporal_ms": {"mean": statistics.mean(times["temporal"]), "stdev": statistics.pstdev(times["temporal"])},
           "svgf_ms": {"mean": statistics.mean(times["svgf"]), "stdev": statistics.pstdev(times["svgf"]), "iterations": art.SVGF_ITERATIONS},
           "floor_ms": W * H * BYTES_PER_PIXEL / (BANDWIDTH_TBS * 1e12) * 1e3, "bytes_per_pixel": BYTES_PER_PIXEL, "bandwidth_TBs": BANDWIDTH_TBS,
           "pixels_with_history": float((found > SPP).float().mean()),
           "set_camera_plus_pass_ms": t_set, "upload_plus_pass_ms": t_up,
           "stage_counts_equal": stages_before == stages_after, "stage_counts": stages_before[:2]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    be.shutdown()


if __name__ == "__main__":
    main()
