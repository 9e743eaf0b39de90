"""First-hit feature buffers on one MI355X: art_render_aovs_device against the way a torch user gets the same data without it.

C4 (scenes.synthetic_scene(1000000, 4)) at 1920 x 1080, anti-aliasing on: 4 x 2 073 600 camera rays.
  (a) aov_ms           GPU time of one render_aovs_torch with all seven planes (HIP events on torch's stream), median of 20 after 5 warm-ups
  (b) query_ms         GPU time of trace_rays_torch on the same rays, already generated and resident (the caller's ray generation, the
                       material look-up and the averaging are NOT in it: the base flatters the old way)
  (c) kernel_ms        the kernels of one call, from a separate `rocprofv3 --kernel-trace --stats` run of this script with --device-only
                       (mean over its calls): k_aov_raygen, k_analytic, the trace kernel, k_aov_resolve.  The call's trace launch is not
                       timed by the library (ArtStats does not see it, as for the device queries), so ArtStats::trace_ms cannot give it.
Reported: (a) / (b); the share of the call's kernel time outside the trace launch (k_analytic + trace kernel); the resolve kernel's
store rate against its algorithmic bytes (44 B stored per pixel; 64 B of hit records read).

usage: python profiles/aov/measure.py --out DIR
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace -- python profiles/aov/measure.py --device-only
       python profiles/aov/measure.py --out DIR --kstats DIR/trace        (folds the kernel times into DIR/measure.json)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
STORED_PER_PIXEL, READ_PER_PIXEL = 44, 64


def setup():
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    be.upload_scene(scenes.synthetic_scene(1000000, 4))
    be.resize(W, H)
    return art, be, art.Backend.pass_params(art.PT_MIS, True, 8, 1)


def gpu_ms(torch, call, n, warm):
    ms = []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def camera_rays(torch, scene_desc):
    """the four rays of every pixel in float32 on the GPU, slot s * npix + pixel (a user's own copy of camera_dir(); near enough for timing)"""
    dev = torch.device("cuda")
    x = torch.arange(W, device=dev, dtype=torch.float32).repeat(H); y = torch.arange(H, device=dev, dtype=torch.float32).repeat_interleave(W)
    out = []
    for s in range(4):
        ox, oy = (1.0 / 3.0, 2.0 / 3.0)[(s >> 1) & 1], (1.0 / 3.0, 2.0 / 3.0)[s & 1]
        d = torch.stack([x + ox - W / 2.0, y + oy - H / 2.0, torch.full_like(x, -float(W))], -1)
        out.append(d / d.norm(dim=1, keepdim=True))
    d = torch.cat(out).contiguous()
    o = torch.tensor(list(scene_desc), device=dev, dtype=torch.float32).repeat(d.shape[0], 1).contiguous()
    return o, d


def measure(args):
    import torch
    art, be, p = setup()
    if args.device_only:
        for _ in range(8):
            be.render_aovs_torch(p)
        torch.cuda.synchronize()
        return
    from ada_ray_tracer_amd import scenes
    a = gpu_ms(torch, lambda: be.render_aovs_torch(p), 20, 5)
    o, d = camera_rays(torch, scenes.REFERENCE_CAMERA)
    b = gpu_ms(torch, lambda: be.trace_rays_torch(o, d), 20, 5)
    planes = be.render_aovs_torch(p)
    hits = be.trace_rays_torch(o, d)
    alpha_q = (hits.is_hit.reshape(4, H, W).float().sum(0) * 0.25)
    res = {"what": "art_render_aovs_device (all planes) against trace_rays_torch on the same 4 x %d camera rays, C4, %d x %d, AA on" % (W * H, W, H),
           "device": torch.cuda.get_device_name(0), "rays": 4 * W * H,
           "aov_ms": {"median": a[0], "min": a[1], "max": a[2]}, "query_ms": {"median": b[0], "min": b[1], "max": b[2]},
           "aov_over_query": a[0] / b[0],
           "alpha_equals_the_queries_is_hit_mean": bool(torch.equal(planes["alpha"], alpha_q)),
           "kernel_ms": None}
    os.makedirs(args.out, exist_ok=True)
    json.dump(res, open(os.path.join(args.out, "measure.json"), "w"), indent=1)
    print(json.dumps(res))


def fold_kstats(args):
    path = os.path.join(args.out, "measure.json")
    res = json.load(open(path))
    files = glob.glob(os.path.join(args.kstats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % args.kstats)
    k = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Name"].split("(")[0].split("<")[0].replace("void ", "").replace("art::", "")
        for key in ("k_aov_raygen", "k_analytic", "k_trace_coop", "k_aov_resolve"):
            if name.endswith(key):
                e = k.setdefault(key, {"calls": 0, "total_ns": 0})
                e["calls"] += int(r["Calls"]); e["total_ns"] += int(r["TotalDurationNs"])
    ms = {key: v["total_ns"] * 1e-6 / max(1, v["calls"]) for key, v in k.items()}
    total = sum(ms.values())
    res["kernel_ms"] = ms
    res["kernel_calls"] = {key: v["calls"] for key, v in k.items()}
    res["share_outside_trace_launch"] = (ms.get("k_aov_raygen", 0.0) + ms.get("k_aov_resolve", 0.0)) / total
    rs = ms.get("k_aov_resolve", 0.0) * 1e-3
    if rs > 0:
        res["resolve_store_GBps"] = STORED_PER_PIXEL * W * H / rs * 1e-9
        res["resolve_load_plus_store_GBps"] = (STORED_PER_PIXEL + READ_PER_PIXEL) * W * H / rs * 1e-9
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "aov"))
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--kstats")
    args = ap.parse_args()
    fold_kstats(args) if args.kstats else measure(args)
