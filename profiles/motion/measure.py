"""The motion plane on one MI355X: what it adds to the feature buffers and to the temporal call.  NOT YET RUN: no measure.json exists.

C4 (scenes.synthetic_scene(1000000, 4)) at 1920 x 1080, anti-aliasing on, the soup moved by one refit; in ONE process, alternating:
  (a) aov_ms / aov_motion_ms            GPU time of render_aovs_torch_motion's call without and with the motion plane (want = albedo, normal,
                                        depth, prim_index; HIP events on torch's stream), median of 20 pairs after 5 warm-ups
  (b) temporal_ms / temporal_motion_ms  the same for art_temporal_motion_device with motion3f NULL and given
The expectation to hold the figures against is the byte count: 12 B of 156 per pixel more for the temporal kernel; one index triple and
six vertices (84 B) per mesh hit, plus 12 B stored per pixel, for the resolve.

usage: python profiles/motion/measure.py --out DIR        (writes DIR/measure.json)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 1920, 1080


def pair_ms(torch, a, b, n=20, warm=5):
    """a and b alternating: their median, min and max GPU times"""
    ms = ([], [])
    for i in range(warm + n):
        for k, call in enumerate((a, b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            if i >= warm:
                ms[k].append(e0.elapsed_time(e1))
    return [{"median": statistics.median(m), "min": min(m), "max": max(m)} for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "motion"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    sd = scenes.synthetic_scene(1000000, 4)
    be.upload_scene(sd); be.resize(W, H)
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1)
    prev = torch.from_numpy(np.ascontiguousarray(sd._mesh_arrays[-1][0], np.float32)).cuda()
    cur = (prev + torch.tensor([0.05, 0.0, 0.02], device="cuda")).contiguous()
    be.refit_torch(cur)
    want = ("albedo", "normal", "depth", "prim_index")
    aov = pair_ms(torch, lambda: be.render_aovs_torch(p, want), lambda: be.render_aovs_torch_motion(p, want, cur_pos=cur, prev_pos=prev))
    planes = be.render_aovs_torch_motion(p, want, cur_pos=cur, prev_pos=prev)
    color = torch.rand((H, W, 3), device="cuda"); moments = torch.rand((H, W, 2), device="cuda")
    cam = (np.array(scenes.REFERENCE_CAMERA, np.float32), np.eye(4, dtype=np.float32))
    frame = dict(planes, color=color, moments=moments)
    hist = be.temporal_torch(frame, None, cam, None, 1)[3]
    tmp = pair_ms(torch, lambda: be.temporal_torch(frame, hist, cam, cam, 1), lambda: be.temporal_torch(frame, hist, cam, cam, 1, motion=planes["motion"]))
    res = {"what": "the motion plane's cost, C4, %d x %d, AA on, alternating in one process" % (W, H), "device": torch.cuda.get_device_name(0),
           "aov_ms": aov[0], "aov_motion_ms": aov[1], "temporal_ms": tmp[0], "temporal_motion_ms": tmp[1],
           "mesh_pixel_share": float((planes["motion"].abs().sum(-1) > 0).float().mean()),
           "expected": {"temporal_bytes_per_pixel": [156, 168], "resolve_extra_bytes_per_mesh_hit": 84, "resolve_extra_store_per_pixel": 12}}
    os.makedirs(args.out, exist_ok=True)
    json.dump(res, open(os.path.join(args.out, "measure.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
