"""The variance-guided denoiser and the moments on one MI355X.

Workload: C4 (scenes.synthetic_scene(1000000, 4)) at 1920 x 1080, accum and moments bound, PT_MIS passes without anti-aliasing
(4 virtual threads: 4 spp and 4 colours per pass, so that one pass gives a variance), render_aovs_torch, 5 iterations of either filter.
  (a) filter_ms   GPU time (HIP events on torch's stream) of art_denoise_svgf_device and of art_denoise_device on the same frame in the
                  same process, the two alternating: 3 warm-up and 20 timed calls each; their ratio.
  (b) fold_ms     the fold group's event pairs (ArtStageStats::fold_ms: k_resolve_last + k_fold_level + k_accumulate or
                  k_accumulate_moments) of 5 passes with moments bound against 5 passes unbound, after one warm-up pass each, alternating.
                  The bound variant adds 8 B read and 8 B written per pixel to the accumulate's rad reads (12 B per sample) and the
                  accum's 12 + 12 B.
  (c) kernel_ms   with --kstats DIR (a rocprofv3 --kernel-trace --stats run of `measure.py --device-only`): time per launch of
                  k_denoise_pack<dn::Mode::Svgf>, k_atrous<true, false>, k_atrous<true, true> next to the plain filter's kernels
                  (k_denoise_pack<dn::Mode::Plain>, k_atrous<false, false>, k_atrous<false, true>).

usage: python profiles/svgf/measure.py --out DIR
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace -- python profiles/svgf/measure.py --device-only
       python profiles/svgf/measure.py --out DIR --kstats DIR/trace"""
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
ITERATIONS = 5


def stat(ms):
    return {"mean": statistics.mean(ms), "stdev": statistics.stdev(ms), "min": min(ms), "max": max(ms), "calls": len(ms)}


def measure(args):
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    be.upload_scene(scenes.synthetic_scene(1000000, 4))
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    p = art.Backend.pass_params(art.PT_MIS, False, 8, 4, seed=7)
    be.bind_accum(accum)

    def passes(n, bound):
        """fold_ms per pass of n passes after a resize and one warm-up pass"""
        be.bind_moments(moments if bound else None)
        be.resize(W, H)
        spp = be.render_pass_device(p, 0)
        be.synchronize()
        f0 = be.stage_stats().fold_ms
        for _ in range(n):
            spp = be.render_pass_device(p, spp)
        be.synchronize()
        return (be.stage_stats().fold_ms - f0) / n, spp
    fold = {"bound": [], "unbound": []}
    for _ in range(3):
        fold["unbound"].append(passes(5, False)[0])
        fold["bound"].append(passes(5, True)[0])
    be.bind_moments(moments)
    be.resize(W, H)
    spp = be.render_pass_device(p, 0)                       # the frame the filters run on: 4 spp, 4 colours
    aovs = be.render_aovs_torch(p, want=("albedo", "normal", "depth"))
    out = torch.empty_like(accum)
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    svgf = lambda: be.denoise_svgf_torch(accum, moments, spp, **aovs, scale=1.0 / spp, iterations=ITERATIONS, sigma_color=2.0, out=out, variance_out=var)
    plain = lambda: be.denoise_torch(accum, **aovs, scale=1.0 / spp, iterations=ITERATIONS, out=out)
    if args.device_only:
        for _ in range(8):
            svgf(); plain()
        torch.cuda.synchronize()
        be.bind_moments(None); be.bind_accum(None)
        return
    ms = {"svgf": [], "plain": []}
    for i in range(3 + 20):
        for name, call in (("svgf", svgf), ("plain", plain)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            if i >= 3:
                ms[name].append(e0.elapsed_time(e1))
    be.bind_moments(None); be.bind_accum(None)
    res = {"what": "art_denoise_svgf_device against art_denoise_device, %d iterations, C4, %d x %d, 4 spp without anti-aliasing (4 colours); "
                   "fold group of a pass with and without moments bound" % (ITERATIONS, W, H),
           "device": torch.cuda.get_device_name(0), "pixels": W * H, "iterations": ITERATIONS,
           "filter_ms": {k: stat(v) for k, v in ms.items()}, "svgf_over_plain": statistics.mean(ms["svgf"]) / statistics.mean(ms["plain"]),
           "fold_ms_per_pass": {k: {"runs_of_5_passes": v, "mean": statistics.mean(v)} for k, v in fold.items()},
           "fold_bound_over_unbound": statistics.mean(fold["bound"]) / statistics.mean(fold["unbound"]),
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
        name = r["Name"].replace("void ", "").replace("art::", "").rsplit("(", 1)[0]      # (a pack kernel's template argument holds a "(" too)
        if name.startswith(("k_denoise_pack", "k_atrous")):
            e = k.setdefault(name, {"calls": 0, "total_ns": 0})
            e["calls"] += int(r["Calls"]); e["total_ns"] += int(r["TotalDurationNs"])
    res["kernel_ms"] = {key: v["total_ns"] * 1e-6 / max(1, v["calls"]) for key, v in k.items()}      # per launch
    res["kernel_calls"] = {key: v["calls"] for key, v in k.items()}
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "svgf"))
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--kstats")
    args = ap.parse_args()
    fold_kstats(args) if args.kstats else measure(args)
