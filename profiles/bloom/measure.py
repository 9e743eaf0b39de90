"""GPU time of art_bloom_device on one MI355X at 1920 x 1080: six levels (the default) and eight, both variants.

One process, the calls alternating round by round (so drift and other tenants hit all of them alike), each timed by device events around
INNER back-to-back calls on torch's stream, as profiles/firefly/measure.py does:
  bloom_6_v0, bloom_6_v1, bloom_8_v0, bloom_8_v1   out3f only; v0: the small levels in one workgroup, v1: one launch per level
  bloom_6_v0_both, bloom_6_v1_both                 out3f and bloom3f
  bloom_6_v0_threshold                             with a soft knee whose exposure is read from a state on the device
  display                                          art_display_device (ACES, sRGB, dither) on the same frame
  denoise_1_iteration                              art_denoise_device with iterations = 1, the yardstick of the other READMEs
against the call's compulsory bytes at 6.3 TB/s (profiles/denoise/README.md): the frame read (12 B per pixel) and written (12 B per
output plane), and the pyramid's 16-byte records written once and read once on the way up.  (The kernels read more: the colour a
second time in the mix, and every record by the level below it as well.)  Every ms figure is an upper bound of the GPU time per call:
where the host issues calls more slowly than the kernels run it is the host's issue rate (host_issue_ms beside it).

"variant_0_wins": per level count, whether variant 0's mean lies below variant 1's by more than the larger of the two standard deviations
over the rounds -- what decides bloom.BLOOM_VARIANT (README.md).

usage: python profiles/bloom/measure.py [--out profiles/bloom/measure.json] [--reps 10] [--inner 20]"""
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
TAIL_TEXELS = 4096


def plan(levels, variant):
    """(records of the pyramid, launches per call, the tail's first level or 0) -- the rule of csrc/art_bloom.h"""
    sizes, w, h = [], W, H
    for _ in range(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        sizes.append(w * h)
        if (w, h) == (1, 1):
            break
    M, tail = len(sizes), 0
    if variant == 0:
        for k in range(1, M):
            if sum(sizes[k - 1:]) <= TAIL_TEXELS:
                tail = k
                break
    return sum(sizes), (2 * tail + 1 if tail else 2 * M), tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom", "measure.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
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
    # a noisy HDR frame with one pixel in 500 a thousand times its surroundings
    color = torch.empty((H, W, 3), device="cuda").uniform_(0.2, 1.0, generator=gen)
    lights = torch.empty((H, W), device="cuda").uniform_(0.0, 1.0, generator=gen) < 0.002
    color = torch.where(lights[..., None], color * 1000.0, color).contiguous()
    out, B, fout = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 3), device="cuda")
    screen = torch.empty((H, W), dtype=torch.int32, device="cuda")
    st = be.exposure_state()
    be.auto_exposure_torch(color, st)
    calls = {}
    for levels in (6, 8):
        for v in (0, 1):
            calls["bloom_%d_v%d" % (levels, v)] = lambda levels=levels, v=v: be.bloom_torch(color, out=out, want_bloom=False, levels=levels, variant=v)
    for v in (0, 1):
        calls["bloom_6_v%d_both" % v] = lambda v=v: be.bloom_torch(color, out=out, bloom_out=B, levels=6, variant=v)
    calls["bloom_6_v0_threshold"] = lambda: be.bloom_torch(color, st, out=out, want_bloom=False, levels=6, variant=0, threshold=1.0, knee=0.5)
    calls["display"] = lambda: be.display_torch(color, st, out=screen)
    calls["denoise_1_iteration"] = lambda: be.denoise_torch(color, normal=normal, depth=depth, iterations=1, out=fout)
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
    # what the timed calls computed, so that a wrong run is seen: both variants give the same words, and the light is all there
    a = be.bloom_torch(color, levels=8, variant=0)
    b = be.bloom_torch(color, levels=8, variant=1)
    torch.cuda.synchronize()
    same = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
    N = W * H
    nbytes, launches, tails = {}, {}, {}
    for name in calls:
        if not name.startswith("bloom"):
            continue
        levels, v = int(name.split("_")[1]), int(name.split("_")[2][1])
        records, launches[name], tails[name] = plan(levels, v)
        nbytes[name] = 12 * N + (24 if name.endswith("both") else 12) * N + 2 * 16 * records
    floors = {k: v / (BANDWIDTH_TBS * 1e12) * 1e3 for k, v in nbytes.items()}
    stat = {k: {"mean": statistics.mean(v), "stdev": statistics.pstdev(v), "min": min(v), "max": max(v)} for k, v in ms.items()}
    dn = stat["denoise_1_iteration"]["mean"]
    wins = {}
    for levels in (6, 8):
        s0, s1 = stat["bloom_%d_v0" % levels], stat["bloom_%d_v1" % levels]
        spread = max(s0["stdev"], s1["stdev"])
        wins[str(levels)] = {"v0_mean": s0["mean"], "v1_mean": s1["mean"], "spread": spread, "variant_0_wins": bool(s1["mean"] - s0["mean"] > spread)}
    res = {"what": "%d x %d, one MI355X; per call, the mean over %d back-to-back calls between two device events; %d rounds after 3 warm ones, "
                   "the calls alternating inside every round" % (W, H, args.inner, args.reps),
           "caveat": "every ms figure is an upper bound of the GPU time per call: where the host issues calls more slowly than the kernels run, "
                     "it is the host's issue rate (host_issue_ms beside it)",
           "ms": stat, "host_issue_ms": {k: statistics.mean(v) for k, v in host.items()}, "launches_per_call": launches, "tail_first_level": tails,
           "compulsory_bytes": nbytes, "floor_ms": floors, "variant_0_against_variant_1": wins,
           "ratio_to_denoise_1_iteration": {k: v["mean"] / dn for k, v in stat.items()},
           "ratio_to_floor": {k: stat[k]["mean"] / floors[k] for k in floors},
           "check": {"finite": bool(torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()), "variants_give_the_same_words": same,
                     "sum_of_bloom_over_sum_of_frame": float(a[1].double().sum() / color.double().sum()), "planted_lights": int(lights.sum()), "pixels": N}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))
    be.shutdown()


if __name__ == "__main__":
    main()
