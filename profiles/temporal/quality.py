"""Which defaults Backend.temporal_torch ships: a sweep of max_history x depth_tol x normal_min on the CPU, before any GPU run.

Frames: tests/temporal_quality.py -- scenes.synthetic_scene(2000, 3) at 48 x 48, PT_MIS, depth 8, no anti-aliasing, four cameras along a
pan, 4 spp each from the CPU oracle (seed 7 + frame); feature buffers from the product's host build.  The reference picture is the oracle's
1024 spp at the LAST camera (seed 11).  Both stages are the numpy references (tests/temporal_ref.py, tests/svgf_var_ref.py with the
filter's shipped iterations and sigma_color), which the kernels equal bit for bit.  RMS over all pixels and channels of (picture -
reference), for the last frame alone, after temporal accumulation, and after accumulation and the filter.

usage: python profiles/temporal/quality.py [--golden tests/golden/temporal_quality_ref_48x48.npy]"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MAX_HISTORY = (4, 8, 16, 64)
DEPTH_TOL = (0.01, 0.05, 0.2)
NORMAL_MIN = (0.5, 0.9, 0.99)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "quality.json"))
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--golden", help="write the reference picture here (the quality tests read it); without it the committed one is read")
    args = ap.parse_args()
    import __graft_entry__ as ge
    art = ge.load_package()
    import temporal_quality as Q
    frames, ref = [], None
    for k in range(Q.FRAMES):
        last = k == Q.FRAMES - 1
        acc, mom, g, r = Q.cpu_frame(art, k, args.reference_spp if (last and args.golden) else 0)
        frames.append((acc, mom, g))
        ref = r if r is not None else ref
    if args.golden:
        np.save(args.golden, ref)
    else:
        ref = Q.reference()
    rows = []
    for mh, dt, nm in itertools.product(MAX_HISTORY, DEPTH_TOL, NORMAL_MIN):
        alone, acc, filt = Q.chain(frames, mh, dt, nm, art.SVGF_ITERATIONS, art.SVGF_SIGMA_COLOR)
        row = {"max_history": mh, "depth_tol": dt, "normal_min": nm, "rms_last_frame": Q.rms(alone, ref), "rms_accumulated": Q.rms(acc, ref), "rms_filtered": Q.rms(filt, ref)}
        row["ratio_accumulated"] = row["rms_accumulated"] / row["rms_last_frame"]
        row["ratio_filtered"] = row["rms_filtered"] / row["rms_last_frame"]
        rows.append(row)
        print("max_history %3d depth_tol %.2f normal_min %.2f: alone %.4f accumulated %.4f filtered %.4f" % (mh, dt, nm, row["rms_last_frame"], row["rms_accumulated"], row["rms_filtered"]), flush=True)
    best = min(rows, key=lambda r: (r["ratio_filtered"], -r["max_history"]))      # (a tie goes to the longer history: four frames of 4 colours cannot tell 16 from 64)
    res = {"what": "RMS error of the last of %d frames of a pan against %d spp at its camera; synthetic_scene(2000, 3), %d x %d, PT_MIS, depth 8, no "
                   "anti-aliasing, %d spp per frame; CPU oracle samples, numpy references (filter: iterations %d, sigma_color %g)"
                   % (Q.FRAMES, args.reference_spp, Q.W, Q.H, Q.SPP, art.SVGF_ITERATIONS, art.SVGF_SIGMA_COLOR),
           "best": best, "asserted_ratio": Q.bound(best), "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("best:", best)


if __name__ == "__main__":
    main()
