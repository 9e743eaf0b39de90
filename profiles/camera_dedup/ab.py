"""A/B of option camera_dedup inside ONE process on the bench workload (C4: 1920x1080, PT_MIS depth 8, AA, 256 spp per step): the two
settings alternate in blocks of --steps steps, so both see the same process, mapping of the path state and clocks.
    python profiles/camera_dedup/ab.py [--rounds 3] [--steps 4] [--warmup 3]
Prints one JSON line per block and a summary line (medians)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--vthreads", type=int, default=64)
    args = ap.parse_args()
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    be.upload_scene(scenes.synthetic_scene(args.tris, 4))
    be.resize(args.width, args.height)
    prm = art.Backend.pass_params(art.PT_MIS, True, 8, args.vthreads, seed=1)
    spp = 0
    for _ in range(args.warmup):
        spp = be.render_pass_device(prm, spp)
    be.synchronize()
    res = {0: [], 1: []}
    for rnd in range(args.rounds):
        for dedup in (1, 0):
            be.set_option("camera_dedup", dedup)
            s0, g0, c0 = be.stats(), be.stage_stats(), be.camera_rays_traced()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                spp = be.render_pass_device(prm, spp)
            be.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            s1, g1, c1 = be.stats(), be.stage_stats(), be.camera_rays_traced()
            row = {"round": rnd, "camera_dedup": dedup, "ms_per_step": round(ms, 2), "trace_ms_per_step": round((s1.trace_ms - s0.trace_ms) / args.steps, 2),
                   "raygen_ms_per_step": round((g1.raygen_ms - g0.raygen_ms) / args.steps, 3), "shade_ms_per_step": round((g1.shade_ms - g0.shade_ms) / args.steps, 2),
                   "rays_per_step": (s1.rays - s0.rays) // args.steps, "camera_rays_traced_per_step": (c1 - c0) // args.steps}
            res[dedup].append(row)
            print(json.dumps(row), flush=True)
    be.set_option("camera_dedup", 1)
    med = {k: {f: statistics.median(r[f] for r in rows) for f in ("ms_per_step", "trace_ms_per_step", "raygen_ms_per_step", "shade_ms_per_step")} for k, rows in res.items()}
    print(json.dumps({"median": {"camera_dedup=1": med[1], "camera_dedup=0": med[0]},
                      "ms_per_step_ratio": round(med[1]["ms_per_step"] / med[0]["ms_per_step"], 4)}))
    be.shutdown()


if __name__ == "__main__":
    main()
