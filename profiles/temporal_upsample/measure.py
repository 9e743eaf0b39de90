"""GPU time of art_temporal_upsample_device on one MI355X: a 960 x 540 frame into a 1920 x 1080 history with every guide, beside the two
calls it stands between.

One process, the calls alternating round by round (so drift and other tenants hit all of them alike), each timed by device events around
INNER back-to-back calls on torch's stream, as profiles/upsample/measure.py does:
  temporal_upsample          normal, depth and id on both sides, a history in and out, every output and the fallback plane, cameras at rest
  temporal_upsample_motion   the same with the hi motion plane (the history is then found through the projection)
  temporal_hi                art_temporal_device at 1920 x 1080 on the hi guides (the accumulation alone, at the size it would be traced at)
  upsample_fp2               art_upsample_device from 960 x 540 with the same guides and albedo (the upsampling alone)
against the call's compulsory bytes at 6.3 TB/s (profiles/denoise/README.md): per hi pixel 137 B (149 B with motion), per lo pixel 136 B
(art_temporal_upsample.hip states the sum).  Every ms figure is an upper bound of the GPU time per call: where the host issues calls more
slowly than the kernels run it is the host's issue rate (host_issue_ms beside it).  No time is asserted anywhere.

usage: python profiles/temporal_upsample/measure.py [--out profiles/temporal_upsample/measure.json] [--reps 10] [--inner 20]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H, LW, LH = 1920, 1080, 960, 540
BANDWIDTH_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_upsample", "measure.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import __graft_entry__ as ge
    art = ge.load_package()
    be = art.Backend(0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)

    def side(w, h):
        """planes of a slanted floor under a wall: a normal crease, a depth step and an id boundary across the frame"""
        y = torch.arange(h, device="cuda", dtype=torch.float32).view(h, 1).expand(h, w) / h
        x = torch.arange(w, device="cuda", dtype=torch.float32).view(1, w).expand(h, w) / w
        wall = (y + 0.1 * x) < 0.45
        normal = torch.zeros((h, w, 3), device="cuda")
        normal[..., 2] = wall.float(); normal[..., 1] = (~wall).float()
        depth = torch.where(wall, 20.0 + x, 5.0 + 10.0 * (1.0 - y)).contiguous()
        ident = (wall.int() * 7 + (x * 40).int()).contiguous()
        albedo = torch.empty((h, w, 3), device="cuda").uniform_(0.05, 1.0, generator=gen)
        return dict(albedo=albedo, normal=normal.contiguous(), depth=depth, id=ident, prim_index=ident)
    lo, hi = side(LW, LH), side(W, H)
    lo_color = torch.exp(torch.empty((LH, LW, 3), device="cuda").uniform_(-4.6, 4.6, generator=gen)).contiguous()
    lo_moments = torch.empty((LH, LW, 2), device="cuda").uniform_(0.1, 4.0, generator=gen)
    hi_color = torch.exp(torch.empty((H, W, 3), device="cuda").uniform_(-4.6, 4.6, generator=gen)).contiguous()
    hi_moments = torch.empty((H, W, 2), device="cuda").uniform_(0.1, 4.0, generator=gen)
    motion = torch.zeros((H, W, 3), device="cuda")
    cam = (np.zeros(3, np.float32), np.eye(4, dtype=np.float32))
    jit = art.temporal_upsample.jitter_sequence(2)[1]
    j = (float(jit[0]), float(jit[1]))
    hist = be.temporal_upsample_torch(lo_color, lo_moments, lo, hi, cam, n_colours=4, scale=0.25)[3]
    hist_t = be.temporal_torch(dict(hi, color=hi_color, moments=hi_moments), None, cam, None, 4, scale=0.25)[3]
    out = torch.empty((H, W, 3), device="cuda")
    calls = {
        "temporal_upsample": lambda: be.temporal_upsample_torch(lo_color, lo_moments, lo, hi, cam, cam, hist, jitter=j, n_colours=4, scale=0.25, want_fallback=True),
        "temporal_upsample_motion": lambda: be.temporal_upsample_torch(lo_color, lo_moments, lo, dict(hi, motion=motion), cam, cam, hist, jitter=j, n_colours=4,
                                                                       scale=0.25, want_fallback=True),
        "temporal_hi": lambda: be.temporal_torch(dict(hi, color=hi_color, moments=hi_moments), hist_t, cam, cam, 4, scale=0.25),
        "upsample_fp2": lambda: be.upsample_torch(lo_color, lo, hi, footprint=2, out=out, want_fallback=True),
    }
    ms, host = {k: [] for k in calls}, {k: [] for k in calls}
    for r in range(args.reps + 3):                                  # three warm rounds: code objects, torch's allocator, the scratch
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            t1 = time.perf_counter()
            e1.record(); e1.synchronize()
            if r >= 3:
                ms[name].append(e0.elapsed_time(e1) / args.inner)
                host[name].append((t1 - t0) * 1e3 / args.inner)
    # what the timed calls computed, so that a wrong run is seen
    res_out, var, length, _, fb = calls["temporal_upsample"]()
    torch.cuda.synchronize()
    N, NL = W * H, LW * LH
    nbytes = {"temporal_upsample": 137 * N + 136 * NL, "temporal_upsample_motion": 149 * N + 136 * NL, "temporal_hi": 156 * N, "upsample_fp2": 45 * N + 108 * NL}
    floors = {k: v / (BANDWIDTH_TBS * 1e12) * 1e3 for k, v in nbytes.items()}
    stat = {k: {"mean": statistics.mean(v), "stdev": statistics.pstdev(v), "min": min(v)} for k, v in ms.items()}
    res = {"what": "%d x %d from %d x %d, one MI355X; per call, the mean over %d back-to-back calls between two device events; %d rounds after 3 "
                   "warm ones, the calls alternating inside every round" % (W, H, LW, LH, args.inner, args.reps),
           "caveat": "every ms figure is an upper bound of the GPU time per call: where the host issues calls more slowly than the kernels run, "
                     "it is the host's issue rate (host_issue_ms beside it)",
           "ms": stat, "host_issue_ms": {k: statistics.mean(v) for k, v in host.items()}, "compulsory_bytes": nbytes, "floor_ms": floors,
           "ratio_to_floor": {k: stat[k]["mean"] / floors[k] for k in stat},
           "check": {"finite": bool(torch.isfinite(res_out).all()), "fallback_pixels": int((fb != 0).sum()), "mean_length": float(length.mean()), "pixels": N}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))
    be.shutdown()


if __name__ == "__main__":
    main()
