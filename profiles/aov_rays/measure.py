"""Feature buffers on one MI355X: art_aovs_rays_device on the frame's own camera rays against art_render_aovs_device.

C4 (scenes.synthetic_scene(1000000, 4)) at 1920 x 1080 with anti-aliasing: 8 294 400 camera rays, all planes.  Alternating in one process,
each call between two events on torch's current stream (the stream both calls are enqueued on):
  (a) rays_ms     aovs_rays_torch(o, d, group=4) on the rays camera_rays_torch(p) made once, all eight planes
  (b) rays7_ms    the same without the position plane: the seven planes render_aovs_torch has
  (c) frame_ms    render_aovs_torch(p), all seven planes
  (d) camera_ms   camera_rays_torch(p) itself
Reported per call: median, min, max, and the spread (max - min) / median; then rays7 / frame and rays / frame.

From the bytes, the expected difference of (b) against (c): the pack kernel reads 24 B per ray that k_aov_raygen does not (it computes its
rays), 199 MB or about 0.03 ms at 6.3 TB/s, and does without camera_dir()'s 60 instructions per ray; the trace launch and the resolve see the same
rays in the same slots.  So the two should be level; (a) adds one float3 plane of stores, 25 MB.  Where the measured ratio is further from 1
than those bytes explain by more than the spread, a `rocprofv3 --kernel-trace --stats` run of --device-only names the launch: k_aov_rays_pack
against k_aov_raygen, k_aov_rays_resolve against k_aov_resolve, the trace kernel in both.

usage: python profiles/aov_rays/measure.py --out DIR [--tris N --width W --height H]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace -- python profiles/aov_rays/measure.py --device-only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def timed(torch, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "aov_rays"))
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    from ada_ray_tracer_amd.aov_rays import RAY_PLANES
    be = art.Backend(0)
    sd = scenes.synthetic_scene(args.tris, 4)
    be.upload_scene(sd)
    W, H = args.width, args.height
    be.resize(W, H)
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1)
    o, d = be.camera_rays_torch(p)
    seven = tuple(n for n in RAY_PLANES if n != "position")
    out8 = be.aovs_rays_torch(o, d, group=4)               # the planes are allocated once: the timed calls write into them
    calls = {"rays": lambda: be.aovs_rays_torch(o, d, group=4, out=out8),
             "rays7": lambda: be.aovs_rays_torch(o, d, group=4, want=seven, out={n: out8[n] for n in seven}),
             "frame": lambda: be.render_aovs_torch(p),
             "camera": lambda: be.camera_rays_torch(p)}
    torch.cuda.synchronize()
    if args.device_only:
        for _ in range(6):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        return
    frame = be.render_aovs_torch(p)
    same = all(bool(torch.equal(out8[n].reshape(frame[n].shape), frame[n])) for n in seven)
    runs = {name: [] for name in calls}
    for i in range(args.warmup + args.steps):
        for name, f in calls.items():
            ms = timed(torch, f)
            if i >= args.warmup:
                runs[name].append(ms)
    res = {"what": "art_aovs_rays_device on art_camera_rays_device's rays against art_render_aovs_device: %d x %d, anti-aliasing on (%d rays), "
                   "synthetic_scene(%d, 4), event time per call, alternating in one process" % (W, H, 4 * W * H, args.tris),
           "device": torch.cuda.get_device_name(0), "rays": 4 * W * H, "steps": args.steps, "planes_equal": same}
    for name, ms in runs.items():
        med = statistics.median(ms)
        res[name + "_ms"] = {"median": med, "min": min(ms), "max": max(ms), "spread": (max(ms) - min(ms)) / med}
    res["rays7_over_frame"] = res["rays7_ms"]["median"] / res["frame_ms"]["median"]
    res["rays_over_frame"] = res["rays_ms"]["median"] / res["frame_ms"]["median"]
    res["expected_extra_ms_from_bytes"] = 24.0 * 4 * W * H / 6.3e12 * 1e3
    os.makedirs(args.out, exist_ok=True)
    json.dump(res, open(os.path.join(args.out, "measure.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
