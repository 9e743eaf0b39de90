"""Which defaults Backend.svgf_spatial_variance_torch ships: a sweep of min_history x sigma_depth x radius, and of the filter's iterations
x sigma_color, on the CPU, before any GPU run.

Frames: tests/svgf_spatial_quality.py -- the scene, size and pan of tests/temporal_quality.py (scenes.synthetic_scene(2000, 3) at 48 x 48,
PT_MIS, depth 8, four cameras) at ONE colour per frame: no anti-aliasing, 1 spp per frame from the CPU oracle (seed 7 + frame) through
tests/moments_ref.py; feature buffers from the product's host build.  The reference pictures are the oracle's 1024 spp (seed 11) at the
SECOND camera, where every history is short, and at the LAST one.  Every stage is a numpy reference the kernels equal bit for bit
(tests/temporal_ref.py with the shipped defaults, tests/svgf_spatial_ref.py, tests/svgf_var_ref.py).  RMS over all pixels and channels
of (filtered picture - reference), WITH the new call between accumulation and filter and WITHOUT it -- the chain as it was -- in the
same run at the same iterations and sigma_color.

usage: python profiles/svgf_spatial/quality.py [--golden tests/golden/svgf_spatial_quality_ref_48x48.npy]"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MIN_HISTORY = (2.0, 3.0, 4.0, 8.0)
SIGMA_DEPTH = (0.0, 1.0, 4.0)
RADIUS = (1, 2, 3)
ITERATIONS = (1, 3, 5)
SIGMA_COLOR = (1.0, 2.0, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf_spatial", "quality.json"))
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--golden", help="write the reference pictures here (the quality tests read them); without it the committed ones are read")
    args = ap.parse_args()
    import __graft_entry__ as ge
    art = ge.load_package()
    import svgf_spatial_quality as Q
    frames, refs = [], {}
    for k in range(Q.FRAMES):
        acc, mom, g, r = Q.cpu_frame(art, k, args.reference_spp if (args.golden and k in (Q.SECOND, Q.LAST)) else 0)
        frames.append((acc, mom, g))
        if r is not None:
            refs[k] = r
    if args.golden:
        np.save(args.golden, np.stack([refs[Q.SECOND], refs[Q.LAST]]))
    else:
        refs[Q.SECOND], refs[Q.LAST] = Q.reference()
    steps = Q.accumulate(art, frames)
    at = {"second": Q.SECOND, "last": Q.LAST}
    short = {name: float(np.mean(~np.isfinite(steps[k][1]))) for name, k in at.items()}
    without, rows = {}, []
    for it, sc in itertools.product(ITERATIONS, SIGMA_COLOR):
        without[(it, sc)] = {name: Q.rms(Q.filtered(steps[k], it, sc)[0], refs[k]) for name, k in at.items()}
        print("without: iterations %d sigma_color %g: second %.4f last %.4f" % (it, sc, without[(it, sc)]["second"], without[(it, sc)]["last"]), flush=True)
    for mh, sd, r in itertools.product(MIN_HISTORY, SIGMA_DEPTH, RADIUS):
        for it, sc in itertools.product(ITERATIONS, SIGMA_COLOR):
            row = {"min_history": mh, "sigma_depth": sd, "radius": r, "iterations": it, "sigma_color": sc}
            for name, k in at.items():
                w = Q.rms(Q.filtered(steps[k], it, sc, dict(radius=r, min_history=mh, sigma_depth=sd))[0], refs[k])
                row["rms_with_" + name], row["rms_without_" + name] = w, without[(it, sc)][name]
                row["ratio_" + name] = w / without[(it, sc)][name]
            rows.append(row)
        b = min(rows[-len(ITERATIONS) * len(SIGMA_COLOR):], key=lambda x: x["ratio_second"])
        print("min_history %g sigma_depth %g radius %d: best ratio second %.4f last %.4f (iterations %d sigma_color %g)"
              % (mh, sd, r, b["ratio_second"], b["ratio_last"], b["iterations"], b["sigma_color"]), flush=True)
    # the filter's shipped iterations and sigma_color stay what profiles/svgf/quality.json chose; among the rows at that setting the best
    # is the lowest ratio at the second frame (every history short: the case the call is for) that does not raise the last frame's error
    mine = [x for x in rows if x["iterations"] == art.SVGF_ITERATIONS and x["sigma_color"] == art.SVGF_SIGMA_COLOR]
    ok = [x for x in mine if x["ratio_last"] <= 1.0] or mine
    best = min(ok, key=lambda x: (x["ratio_second"], x["ratio_last"], -x["radius"]))
    overall = min(rows, key=lambda x: x["rms_with_second"])
    res = {"what": "RMS error of the filtered second and last of %d frames of a pan against %d spp at their cameras, with and without "
                   "art_svgf_spatial_variance_device between accumulation and filter; synthetic_scene(2000, 3), %d x %d, PT_MIS, depth 8, no "
                   "anti-aliasing, 1 spp = one colour per frame; CPU oracle samples, numpy references (temporal: max_history %d, depth_tol %g, "
                   "normal_min %g)" % (Q.FRAMES, args.reference_spp, Q.W, Q.H, art.TEMPORAL_MAX_HISTORY, art.TEMPORAL_DEPTH_TOL, art.TEMPORAL_NORMAL_MIN),
           "share_of_pixels_without_a_finite_variance": short,
           "best": best, "asserted_ratio_second": Q.bound(best["ratio_second"]), "asserted_ratio_last": Q.bound(best["ratio_last"]),
           "lowest_rms_second_over_all_rows": overall, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("best:", best)
    print("lowest second-frame RMS over all rows:", overall)


if __name__ == "__main__":
    main()
