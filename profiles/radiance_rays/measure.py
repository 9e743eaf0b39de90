"""Radiance queries on one MI355X: art_radiance_rays_device against art_render_pass over the same paths.

C4 (scenes.synthetic_scene(1000000, 4)) at 1920 x 1080 without anti-aliasing: 2 073 600 rays equal to the frame's camera rays (a
user's own float32 copy of camera_dir(): near enough for timing), 4 samples each, PT_MIS, depth 8.  Alternating in one process:
  (a) call_ms    radiance_rays_torch(o, d, samples=4)                    } GPU time between two events on the null stream, which is the
  (b) pass_ms    render_pass_device(pass_params(PT_MIS, False, 8, 4))    } library's stream here; both calls wait at their end
  (c) stage_ms   what the library's own event pairs give per call (art_get_stats / art_get_stage_stats deltas): raygen (k_raygen_rays
                 alone, or k_raygen), shade, trace kernel, fold group (the fold levels + k_accumulate_rays, or + k_accumulate)
Reported: (a) / (b); raygen's share of the call, and the fold group's; the same figures of the pass next to them.  The accumulate
kernel's own time is the difference of the two fold groups at best: a `rocprofv3 --kernel-trace --stats` run of --device-only gives it
exactly (k_raygen_rays, k_accumulate_rays against the call's total).

From the code, the expected extra of (a): 24 B read and about 60 B written per slot in raygen, a bounce 0 that reads its ray instead of
recomputing it, and camera rays that are traced once per sample instead of once per pixel.

usage: python profiles/radiance_rays/measure.py --out DIR [--tris N --width W --height H]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace -- python profiles/radiance_rays/measure.py --device-only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SAMPLES, DEPTH = 4, 8


def camera_rays(torch, cam_pos, W, H):
    dev = torch.device("cuda")
    x = torch.arange(W, device=dev, dtype=torch.float32).repeat(H); y = torch.arange(H, device=dev, dtype=torch.float32).repeat_interleave(W)
    d = torch.stack([x + 0.5 - W / 2.0, y + 0.5 - H / 2.0, torch.full_like(x, -float(W))], -1)
    d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    o = torch.tensor(list(cam_pos), device=dev, dtype=torch.float32).repeat(d.shape[0], 1).contiguous()
    return o, d


def stage_figures(be):
    s, g = be.stats(), be.stage_stats()
    return {"raygen_ms": g.raygen_ms, "shade_ms": g.shade_ms, "fold_ms": g.fold_ms, "trace_ms": s.trace_ms, "rays": s.rays}


def timed(torch, be, call):
    before = stage_figures(be)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record(); e1.synchronize()
    after = stage_figures(be)
    return e0.elapsed_time(e1), {k: after[k] - before[k] for k in before}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "radiance_rays"))
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    sd = scenes.synthetic_scene(args.tris, 4)
    be.upload_scene(sd)
    W, H = args.width, args.height
    be.resize(W, H)
    o, d = camera_rays(torch, sd.desc.cam_pos, W, H)
    out = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    p = art.Backend.pass_params(art.PT_MIS, False, DEPTH, SAMPLES)
    state = {"spp": 0, "base": 0}

    def call():
        be.radiance_rays_torch(o, d, render_type=art.PT_MIS, max_depth=DEPTH, samples=SAMPLES, sample_base=state["base"], out=out)
        state["base"] += SAMPLES

    def full_pass():
        state["spp"] = be.render_pass_device(p, state["spp"])
    if args.device_only:
        for _ in range(6):
            call()
        torch.cuda.synchronize()
        return
    runs = {"call": [], "pass": []}
    for i in range(args.warmup + args.steps):
        for name, f in (("call", call), ("pass", full_pass)):
            ms, stages = timed(torch, be, f)
            if i >= args.warmup:
                runs[name].append((ms, stages))
    res = {"what": "art_radiance_rays_device against art_render_pass over the same paths: %d x %d camera rays without anti-aliasing, %d samples, PT_MIS, depth %d, "
                   "synthetic_scene(%d, 4)" % (W, H, SAMPLES, DEPTH, args.tris),
           "device": torch.cuda.get_device_name(0), "rays": W * H, "samples": SAMPLES, "steps": args.steps}
    for name in runs:
        ms = [r[0] for r in runs[name]]
        stages = {k: statistics.median(r[1][k] for r in runs[name]) for k in runs[name][0][1]}
        res[name] = {"ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}, "stages": stages,
                     "raygen_share": stages["raygen_ms"] / statistics.median(ms), "fold_group_share": stages["fold_ms"] / statistics.median(ms)}
    res["call_over_pass"] = res["call"]["ms"]["median"] / res["pass"]["ms"]["median"]
    os.makedirs(args.out, exist_ok=True)
    json.dump(res, open(os.path.join(args.out, "measure.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
