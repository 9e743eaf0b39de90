"""The a-trous denoiser on one MI355X: art_denoise_device behind a render pass and the feature buffers.

C4 (scenes.synthetic_scene(1000000, 4)) at 1920 x 1080, anti-aliasing on, one PT_MIS pass (4 spp) into a bound torch tensor, then
render_aovs_torch, then denoise_torch(accum, **aovs, scale=1/4) with 5 iterations.
  (a) denoise_ms     GPU time of one denoise_torch call (HIP events on torch's stream): mean, standard deviation, min and max of 20 calls
                     after 3 warm-ups
  (b) aovs_ms        the same for render_aovs_torch (albedo, normal, depth) on the same frame: the call a user pays next to it
  (c) floor_ms       the call's compulsory traffic at the HBM rate MI355X_MICROARCH gives as achievable (6.3 TB/s): per pixel 40 B read
                     (colour, albedo, normal, depth) and 12 B written.  What the kernels move on top of that (the 16-byte records of
                     csrc/art_denoise.h, written once and read by 25 taps per iteration) is the implementation's, not the problem's.
  (d) kernel_ms      per kernel, from a separate `rocprofv3 --kernel-trace --stats` run of this script with --device-only (mean over its calls)
  (e) rms            informative, not a test: scenes.synthetic_scene(2000, 3) at 48 x 48, RMS error against a 1024-spp render of the 4-spp
                     picture before and after the filter

usage: python profiles/denoise/measure.py --out DIR
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace -- python profiles/denoise/measure.py --device-only
       python profiles/denoise/measure.py --out DIR --kstats DIR/trace        (folds the kernel times into DIR/measure.json)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
READ_PER_PIXEL, WRITTEN_PER_PIXEL, HBM_BYTES_PER_S = 40, 12, 6.3e12
ITERATIONS = 5


def frame(art, be, torch, scene, w, h, passes=1, seed=7):
    """(accum tensor, spp, feature buffers) of `passes` PT_MIS passes with AA on"""
    be.upload_scene(scene)
    accum = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    be.bind_accum(accum)
    be.resize(w, h)
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=seed)
    spp = 0
    for _ in range(passes):
        spp = be.render_pass_device(p, spp)
    return accum, spp, p


def gpu_ms(torch, call, n, warm):
    ms = []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return {"mean": statistics.mean(ms), "stdev": statistics.stdev(ms), "min": min(ms), "max": max(ms), "calls": n}


def measure(args):
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    accum, spp, p = frame(art, be, torch, scenes.synthetic_scene(1000000, 4), W, H)
    want = ("albedo", "normal", "depth")
    aovs = be.render_aovs_torch(p, want=want)
    out = torch.empty_like(accum)
    denoise = lambda: be.denoise_torch(accum, **aovs, scale=1.0 / spp, iterations=ITERATIONS, out=out)
    if args.device_only:
        for _ in range(8):
            denoise()
        torch.cuda.synchronize()
        be.bind_accum(None)
        return
    d = gpu_ms(torch, denoise, 20, 3)
    a = gpu_ms(torch, lambda: be.render_aovs_torch(p, want=want), 20, 3)
    floor_ms = (READ_PER_PIXEL + WRITTEN_PER_PIXEL) * W * H / HBM_BYTES_PER_S * 1e3
    be.bind_accum(None)
    # (e) the informative RMS figure on the small scene
    sd = scenes.synthetic_scene(2000, 3)
    acc, s4, p = frame(art, be, torch, sd, 48, 48)
    noisy = acc / s4
    filtered = be.denoise_torch(acc, **be.render_aovs_torch(p, want=want), scale=1.0 / s4, iterations=ITERATIONS)
    torch.cuda.synchronize()
    noisy, filtered = noisy.clone(), filtered.clone()
    be.bind_accum(None)
    ref, sref, _ = frame(art, be, torch, sd, 48, 48, passes=256, seed=11)      # (another seed: the 4 samples are not among the 1024)
    ref = ref / sref
    rms = lambda x: float(((x - ref) ** 2).mean().sqrt())
    res = {"what": "art_denoise_device, %d iterations, behind one 4-spp PT_MIS pass and render_aovs_torch, C4, %d x %d, AA on" % (ITERATIONS, W, H),
           "device": torch.cuda.get_device_name(0), "pixels": W * H, "iterations": ITERATIONS,
           "denoise_ms": d, "aovs_ms": a, "denoise_over_aovs": d["mean"] / a["mean"],
           "floor_ms_at_6.3_TBps": floor_ms, "denoise_over_floor": d["mean"] / floor_ms,
           "rms_48x48": {"reference_spp": sref, "noisy_4spp": rms(noisy), "filtered_4spp": rms(filtered)},
           "kernel_ms": None}
    be.bind_accum(None)
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
        name = r["Name"].replace("void ", "").replace("art::", "").rsplit("(", 1)[0]      # (the pack kernel's template argument holds a "(" too)
        if name.startswith("k_denoise_pack") or name.startswith("k_atrous"):
            e = k.setdefault(name, {"calls": 0, "total_ns": 0})
            e["calls"] += int(r["Calls"]); e["total_ns"] += int(r["TotalDurationNs"])
    res["kernel_ms"] = {key: v["total_ns"] * 1e-6 / max(1, v["calls"]) for key, v in k.items()}      # per launch
    res["kernel_calls"] = {key: v["calls"] for key, v in k.items()}
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "denoise"))
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--kstats")
    args = ap.parse_args()
    fold_kstats(args) if args.kstats else measure(args)
