"""Guided upsampling against plain interpolation on the 48 x 48 test scene, on the CPU: the oracle's samples and the numpy reference
(tests/upsample_ref.py), against the oracle's 1024-spp picture (tests/golden/temporal_quality_ref_48x48.npy).

  (a) 24 x 24 at 16 spp, upsampled under the feature buffers of both resolutions: a sweep over footprint, sigma_depth, normal_log2 and ids
  (b) the same lo frame upsampled with no guide (plain bilinear, footprint 2)
  (c) 48 x 48 at 4 spp, the same ray budget, as it is

The number that matters is (a) / (b).  Where it is below 1 the best setting becomes the default of upsample_torch and the tests assert
guided < ((1 + r) / 2) * unguided (tests/test_upsample_quality.py, tests/test_gpu_upsample.py); (c) is recorded beside both.

usage: python profiles/upsample/quality.py        (writes profiles/upsample/quality.json)
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import __graft_entry__ as ge
    art = ge.load_package()
    import upsample_quality as UQ
    import upsample_ref as U
    ref = UQ.reference().astype("float64")
    lo_color, lo = UQ.cpu_frame(art, UQ.LW, UQ.LH, UQ.LO_SPP)
    same_budget, hi = UQ.cpu_frame(art, UQ.W, UQ.H, UQ.HI_SPP)
    unguided = UQ.rms(U.upsample(lo_color, size=(UQ.W, UQ.H), footprint=2, demodulate=False)[0], ref)
    rows = []
    for fp, sd, nl, ids, demod in itertools.product((2, 4), (0.0, 0.25, 1.0, 4.0, 16.0), (0, 3, 5, 7), (False, True), (False, True)):
        names = ("albedo", "normal", "depth") + (("id",) if ids else ())
        out, fb = U.upsample(lo_color, U.subset(lo, names), U.subset(hi, names), footprint=fp, sigma_depth=sd, normal_log2=nl, demodulate=demod)
        rows.append(dict(footprint=fp, sigma_depth=sd, normal_log2=nl, ids=ids, demodulate=demod, rms=UQ.rms(out, ref), fallback_pixels=int((fb != 0).sum())))
    best = min(rows, key=lambda r: r["rms"])
    rec = dict(scene="scenes.synthetic_scene(2000, 3), camera %d of tests/temporal_quality.py, PT_MIS, depth 8, no anti-aliasing" % UQ.K,
               reference="tests/golden/temporal_quality_ref_48x48.npy (1024 spp)", lo="%d x %d at %d spp" % (UQ.LW, UQ.LH, UQ.LO_SPP),
               hi="%d x %d" % (UQ.W, UQ.H), rms_unguided=unguided, rms_same_budget_full_resolution=UQ.rms(same_budget, ref),
               best=dict(best, ratio=best["rms"] / unguided), sweep=rows)
    with open(os.path.join(ROOT, "profiles", "upsample", "quality.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "sweep"}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
