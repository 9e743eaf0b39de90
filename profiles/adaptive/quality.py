"""Which defaults Backend.render_adaptive ships: a sweep of threshold x lum_floor x min_colours on the CPU, before any GPU run.

The adaptive loop (tests/adaptive_ref.adaptive_loop: the numpy reference of art_adaptive_estimate_device drives it) runs on the CPU oracle's
own samples of tests/adaptive_quality.py's scene: pixel q takes sample indices spp .. spp + S - 1 in the passes that select it.  Figure:
RMS over all pixels and channels of (mean picture - the 1024-spp reference), adaptive against uniform sampling with the whole budget.  A
setting whose loop ends with an empty mask before 90 % of the budget is spent is recorded but cannot be the best: the comparison is at an
equal number of samples.

usage: python profiles/adaptive/quality.py"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
THRESHOLD = (0.01, 0.02, 0.05, 0.1, 0.2)
LUM_FLOOR = (0.01, 0.1, 1.0)
MIN_COLOURS = (4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "quality.json"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    art = ge.load_package()
    import adaptive_quality as Q
    rad, ref = Q.radiance(art), Q.reference()
    uniform = Q.rms(Q.uniform_picture(rad), ref)
    print("uniform %d spp: RMS %.5f" % (Q.BUDGET_SPP, uniform), flush=True)
    rows = []
    for thr, fl, mc in itertools.product(THRESHOLD, LUM_FLOOR, MIN_COLOURS):
        mean, counts, passes = Q.adaptive_picture(rad, thr, fl, mc)
        used = int(counts.sum())
        row = {"threshold": thr, "lum_floor": fl, "min_colours": mc, "rms_adaptive": Q.rms(mean, ref), "samples": used, "passes": passes,
               "max_count": int(counts.max()), "min_count": int(counts.min()), "budget_spent": used >= 0.9 * Q.BUDGET}
        row["ratio"] = row["rms_adaptive"] / uniform
        rows.append(row)
        print("threshold %.2f lum_floor %.2f min_colours %2d: RMS %.5f ratio %.3f samples %d of %d, %d passes, counts %d..%d"
              % (thr, fl, mc, row["rms_adaptive"], row["ratio"], used, Q.BUDGET, passes, row["min_count"], row["max_count"]), flush=True)
    best = min((r for r in rows if r["budget_spent"]), key=lambda r: r["ratio"])
    res = {"what": "RMS error against 1024 spp of adaptive sampling (a full pass of %d samples, masked passes of %d, at most %d per pixel) and of uniform "
                   "sampling at %d spp, both within a budget of %d samples; synthetic_scene(2000, 3), %d x %d, PT_MIS, depth 8, no anti-aliasing, seed %d; "
                   "CPU oracle samples, numpy reference of the estimate" % (Q.FIRST_VTHREADS, Q.STEP_VTHREADS, Q.MAX_SAMPLES, Q.BUDGET_SPP, Q.BUDGET, Q.W, Q.H, Q.SEED),
           "rms_uniform": uniform, "best": best, "asserted_ratio": Q.bound(best) if best["ratio"] < 1 else None, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("best:", best)


if __name__ == "__main__":
    main()
