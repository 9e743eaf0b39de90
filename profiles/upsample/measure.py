"""GPU time of art_upsample_device on one MI355X: 1920 x 1080 from 960 x 540 with every guide, both footprints.

One process, the calls alternating round by round (so drift and other tenants hit all of them alike), each timed by device events around
INNER back-to-back calls on torch's stream, as profiles/display/measure.py does:
  upsample_fp2          footprint 2, albedo, normal, depth and id given, demodulation, the fallback plane written
  upsample_fp4          the same with footprint 4
  upsample_fp2_no_guide footprint 2 with no guide at all (plain bilinear)
  denoise_1_iteration   art_denoise_device with iterations = 1 on the hi frame, the yardstick of the other READMEs
against the call's compulsory bytes at 6.3 TB/s (profiles/denoise/README.md): per hi pixel 12 B of out3f, 1 B of fallback1b and 32 B of hi
guides; per lo pixel 40 B read by the pack kernel, 32 B of records written, 32 B read once, and 4 B of id.  Every ms figure is an upper
bound of the GPU time per call: where the host issues calls more slowly than the kernels run it is the host's issue rate
(host_issue_ms beside it).

usage: python profiles/upsample/measure.py [--out profiles/upsample/measure.json] [--reps 10] [--inner 20]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample", "measure.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
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
        return dict(albedo=albedo, normal=normal.contiguous(), depth=depth, id=ident)
    lo, hi = side(LW, LH), side(W, H)
    lo_color = torch.exp(torch.empty((LH, LW, 3), device="cuda").uniform_(-4.6, 4.6, generator=gen)).contiguous()
    hi_color = torch.exp(torch.empty((H, W, 3), device="cuda").uniform_(-4.6, 4.6, generator=gen)).contiguous()
    out, fout = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 3), device="cuda")
    calls = {
        "upsample_fp2": lambda: be.upsample_torch(lo_color, lo, hi, footprint=2, out=out, want_fallback=True),
        "upsample_fp4": lambda: be.upsample_torch(lo_color, lo, hi, footprint=4, out=out, want_fallback=True),
        "upsample_fp2_no_guide": lambda: be.upsample_torch(lo_color, {}, {}, footprint=2, out=out),
        "denoise_1_iteration": lambda: be.denoise_torch(hi_color, albedo=hi["albedo"], normal=hi["normal"], depth=hi["depth"], iterations=1, out=fout),
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
    res_out, fb = be.upsample_torch(lo_color, lo, hi, footprint=2, want_fallback=True)
    torch.cuda.synchronize()
    N, NL = W * H, LW * LH
    nbytes = {"upsample_all_guides": 45 * N + 108 * NL, "upsample_no_guide": 12 * N + 76 * NL}
    floors = {k: v / (BANDWIDTH_TBS * 1e12) * 1e3 for k, v in nbytes.items()}
    stat = {k: {"mean": statistics.mean(v), "stdev": statistics.pstdev(v), "min": min(v)} for k, v in ms.items()}
    dn = stat["denoise_1_iteration"]["mean"]
    res = {"what": "%d x %d from %d x %d, one MI355X; per call, the mean over %d back-to-back calls between two device events; %d rounds after 3 "
                   "warm ones, the calls alternating inside every round" % (W, H, LW, LH, args.inner, args.reps),
           "caveat": "every ms figure is an upper bound of the GPU time per call: where the host issues calls more slowly than the kernels run, "
                     "it is the host's issue rate (host_issue_ms beside it)",
           "ms": stat, "host_issue_ms": {k: statistics.mean(v) for k, v in host.items()}, "compulsory_bytes": nbytes, "floor_ms": floors,
           "ratio_to_denoise_1_iteration": {k: v["mean"] / dn for k, v in stat.items()},
           "ratio_to_floor": {"upsample_fp2": stat["upsample_fp2"]["mean"] / floors["upsample_all_guides"],
                              "upsample_fp4": stat["upsample_fp4"]["mean"] / floors["upsample_all_guides"],
                              "upsample_fp2_no_guide": stat["upsample_fp2_no_guide"]["mean"] / floors["upsample_no_guide"]},
           "check": {"finite": bool(torch.isfinite(res_out).all()), "fallback_pixels": int((fb != 0).sum()), "pixels": N}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))
    be.shutdown()


if __name__ == "__main__":
    main()
