"""GPU time of art_firefly_device on one MI355X at 1920 x 1080: both radii, with and without moments and id.

One process, the calls alternating round by round (so drift and other tenants hit all of them alike), each timed by device events around
INNER back-to-back calls on torch's stream, as profiles/upsample/measure.py does:
  firefly_r1, firefly_r2                 colour only, the flag plane written
  firefly_r1_moments_id, firefly_r2_moments_id   with the moments (read and written) and an id plane
  firefly_r2_in_place                    radius 2 with moments and id, out3f = color3f and moments_out2f = moments2f
  temporal                               art_temporal_device with a history, normal, depth and id, between equal cameras
  denoise_1_iteration                    art_denoise_device with iterations = 1, the yardstick of the other READMEs
against the call's compulsory bytes at 6.3 TB/s (profiles/denoise/README.md): per pixel 44 B (the colour read by both kernels, the colour
written, the key written and read), 16 B more with moments, 4 B more with an id, 1 B for the flag.  Every ms figure is an upper bound of
the GPU time per call: where the host issues calls more slowly than the kernels run it is the host's issue rate (host_issue_ms beside it).

usage: python profiles/firefly/measure.py [--out profiles/firefly/measure.json] [--reps 10] [--inner 20]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
BANDWIDTH_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "firefly", "measure.json"))
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
    y = torch.arange(H, device="cuda", dtype=torch.float32).view(H, 1).expand(H, W) / H
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, W).expand(H, W) / W
    wall = (y + 0.1 * x) < 0.45
    normal = torch.zeros((H, W, 3), device="cuda")
    normal[..., 2] = wall.float(); normal[..., 1] = (~wall).float()
    normal = normal.contiguous()
    depth = torch.where(wall, 20.0 + x, 5.0 + 10.0 * (1.0 - y)).contiguous()
    ident = (wall.int() * 7 + (x * 40).int()).contiguous()
    # a noisy frame with one pixel in 500 a hundred times its surroundings
    color = torch.empty((H, W, 3), device="cuda").uniform_(0.2, 1.0, generator=gen)
    spikes = torch.empty((H, W), device="cuda").uniform_(0.0, 1.0, generator=gen) < 0.002
    color = torch.where(spikes[..., None], color * 100.0, color).contiguous()
    lum = 0.2126 * color[..., 0] + 0.7152 * color[..., 1] + 0.0722 * color[..., 2]
    moments = torch.stack([lum, lum * lum], -1).contiguous()
    out, mout, fout = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 2), device="cuda"), torch.empty((H, W, 3), device="cuda")
    c2, m2 = color.clone(), moments.clone()
    cam = (np.array([0.0, 2.55, 12.5], np.float32), np.eye(4, dtype=np.float32))
    cur = dict(color=color, moments=moments, normal=normal, depth=depth, prim_index=ident)
    hist = be.temporal_torch(cur, None, cam, None, 1)[3]
    kw = dict(rank=2, gain=2.0, floor=0.0)
    calls = {
        "firefly_r1": lambda: be.firefly_torch(color, radius=1, out=out, **kw),
        "firefly_r2": lambda: be.firefly_torch(color, radius=2, out=out, **kw),
        "firefly_r1_moments_id": lambda: be.firefly_torch(color, moments, ident, radius=1, out=out, moments_out=mout, **kw),
        "firefly_r2_moments_id": lambda: be.firefly_torch(color, moments, ident, radius=2, out=out, moments_out=mout, **kw),
        "firefly_r2_in_place": lambda: be.firefly_torch(c2, m2, ident, radius=2, out=c2, moments_out=m2, **kw),
        "temporal": lambda: be.temporal_torch(cur, hist, cam, cam, 1),
        "denoise_1_iteration": lambda: be.denoise_torch(color, normal=normal, depth=depth, iterations=1, out=fout),
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
    res_out, res_m, flags = be.firefly_torch(color, moments, ident, radius=2, **kw)
    torch.cuda.synchronize()
    N = W * H
    per_pixel = {"firefly_r1": 45, "firefly_r2": 45, "firefly_r1_moments_id": 65, "firefly_r2_moments_id": 65, "firefly_r2_in_place": 65}
    nbytes = {k: v * N for k, v in per_pixel.items()}
    floors = {k: v / (BANDWIDTH_TBS * 1e12) * 1e3 for k, v in nbytes.items()}
    stat = {k: {"mean": statistics.mean(v), "stdev": statistics.pstdev(v), "min": min(v)} for k, v in ms.items()}
    dn = stat["denoise_1_iteration"]["mean"]
    res = {"what": "%d x %d, one MI355X; per call, the mean over %d back-to-back calls between two device events; %d rounds after 3 warm ones, "
                   "the calls alternating inside every round" % (W, H, args.inner, args.reps),
           "caveat": "every ms figure is an upper bound of the GPU time per call: where the host issues calls more slowly than the kernels run, "
                     "it is the host's issue rate (host_issue_ms beside it)",
           "ms": stat, "host_issue_ms": {k: statistics.mean(v) for k, v in host.items()}, "compulsory_bytes": nbytes, "floor_ms": floors,
           "ratio_to_denoise_1_iteration": {k: v["mean"] / dn for k, v in stat.items()},
           "ratio_to_floor": {k: stat[k]["mean"] / floors[k] for k in floors},
           "check": {"finite": bool(torch.isfinite(res_out).all() and torch.isfinite(res_m).all()), "clamped_pixels": int((flags == 1).sum()),
                     "planted_spikes": int(spikes.sum()), "pixels": N}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))
    be.shutdown()


if __name__ == "__main__":
    main()
