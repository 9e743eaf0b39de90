"""GPU time of the adaptive-sampling calls, measured once on one MI355X.

Workload: C4 (scenes.synthetic_scene(1000000, 4)) at 1920 x 1080, accum and moments bound, PT_MIS, depth 8, 4 spp per pass without
anti-aliasing.
  (a) art_compact_mask_device (its three launches together: torch events around the call) on a random 30 % mask, against the byte floors
      of its launches at the 6.3 TB/s profiles/denoise/ measured: count reads 5 B per pixel, scatter reads 5 B per pixel and writes 4 B
      per selected pixel, the scan moves 8 B per 256 pixels.
  (b) art_adaptive_estimate_device with every output, against its 24 + 21 B per pixel.
  (c) a masked pass with random and with tile-aligned (whole 32 x 32 tiles) masks of 100, 50, 25 and 5 %, against the full pass of the
      same process: host clock around the call, which ends in a synchronise like art_render_pass (it includes the list's read-back).

usage: python profiles/adaptive/measure.py [--out profiles/adaptive/measure.json] [--reps 10]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H, SPP = 1920, 1080, 4
BANDWIDTH_TBS = 6.3          # profiles/denoise/README.md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "measure.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    be.upload_scene(scenes.synthetic_scene(1000000, 4))
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    counts = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    p = art.Backend.pass_params(art.PT_MIS, False, 8, SPP, seed=7)
    be.bind_accum(accum); be.bind_moments(moments)
    be.resize(W, H)
    spp = 0
    for _ in range(3):                                      # warm: code objects, the path state, the shade stage's trial
        spp = be.render_pass_device(p, spp)
    counts += spp
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    N = W * H
    floor = lambda nbytes: nbytes / (BANDWIDTH_TBS * 1e12) * 1e3

    def events(fn):
        ms = []
        for r in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if r >= 3:
                ms.append(e0.elapsed_time(e1))
        return {"mean": statistics.mean(ms), "stdev": statistics.pstdev(ms), "min": min(ms)}

    m30 = (torch.rand((H, W), device="cuda", generator=gen) < 0.3).to(torch.uint8)
    sel = int(m30.count_nonzero())
    res = {"what": "C4 at %d x %d, %d spp per pass, no anti-aliasing; one MI355X; %d repetitions after 3 warm ones" % (W, H, SPP, args.reps)}
    res["compact_ms"] = events(lambda: be.compact_mask_torch(m30))
    res["compact_floor_ms"] = {"count": floor(5 * N), "scan": floor(8 * ((N + 255) // 256)), "scatter": floor(5 * N + 4 * sel), "selected": sel}
    res["estimate_ms"] = events(lambda: be.adaptive_estimate_torch(accum, moments, counts, False))
    res["estimate_floor_ms"] = floor(45 * N)

    def wall(fn):
        ms = []
        for r in range(args.reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            if r >= 1:
                ms.append((time.perf_counter() - t0) * 1e3)
        return {"mean": statistics.mean(ms), "stdev": statistics.pstdev(ms), "min": min(ms)}

    state = {"spp": spp}

    def full():
        state["spp"] = be.render_pass_device(p, state["spp"])

    def masked(mask):
        state["spp"], _ = be.render_pass_masked(p, state["spp"], mask, counts)
    res["full_pass_ms"] = wall(full)
    res["masked_pass_ms"] = {}
    ty, tx = (H + 31) // 32, (W + 31) // 32
    for share in (1.0, 0.5, 0.25, 0.05):
        rnd = (torch.rand((H, W), device="cuda", generator=gen) < share).to(torch.uint8)
        tiles = (torch.rand((ty, tx), device="cuda", generator=gen) < share).to(torch.uint8)
        til = tiles.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W].contiguous()
        for kind, mask in (("random", rnd), ("tiles", til)):
            r = wall(lambda: masked(mask))
            r["selected_share"] = float(mask.count_nonzero()) / N
            res["masked_pass_ms"]["%s_%g" % (kind, share)] = r
    res["full_pass_after_ms"] = wall(full)
    res["lost_paths"] = int(be.stats().lost_paths)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    be.shutdown()


if __name__ == "__main__":
    main()
