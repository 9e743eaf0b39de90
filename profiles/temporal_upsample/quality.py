"""Temporal super-resolution against its two neighbours on the 48 x 48 test scene, on the CPU: the oracle's samples and the numpy
references, against the oracle's 1024-spp picture (tests/golden/temporal_quality_ref_48x48.npy).  tests/temporal_upsample_quality.py
states the inputs and the three chains:

  (A) 8 jittered 24 x 24 frames at 4 spp accumulated into a 48 x 48 history: a sweep over radius, min_confidence and demodulation
  (B) the last of those frames alone through guided upsampling
  (C) the same 8 frames, unjittered, accumulated at 24 x 24 and upsampled once

A / B is what the tests assert at the halfway bound ((1 + r) / 2); A / C says whether super-resolution beats plain accumulation on this
scene and is asserted the same way only where it is below 1.  The best radius and min_confidence become the defaults of
temporal_upsample_torch.

usage: python profiles/temporal_upsample/quality.py        (writes profiles/temporal_upsample/quality.json)
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
    import temporal_upsample_quality as TQ
    import temporal_upsample_ref as R
    ref = TQ.reference().astype("float64")
    b, c = TQ.rms(TQ.chain_b(art), ref), TQ.rms(TQ.chain_c(art), ref)
    rows = []
    for radius, minc, demod in itertools.product((0.5, 0.75, 1.0, 1.25, 1.5, 2.0), (0.0078125, 0.015625, 0.03125, 0.0625, 0.125, 0.25, 0.5, 1.0), (False, True)):
        per_frame = [TQ.rms(TQ.chain_a(R.temporal_upsample, art, radius, minc, demod, frames=n), ref) for n in (1, 2, 4)]
        a = TQ.rms(TQ.chain_a(R.temporal_upsample, art, radius, minc, demod), ref)
        rows.append(dict(radius=radius, min_confidence=minc, demodulate=demod, rms=a, rms_after_1_2_4_frames=per_frame))
    best = min(rows, key=lambda r: r["rms"])
    rec = dict(scene="scenes.synthetic_scene(2000, 3), camera %d of tests/temporal_quality.py at rest, PT_MIS, depth 8, no anti-aliasing" % TQ.K,
               reference="tests/golden/temporal_quality_ref_48x48.npy (1024 spp)", lo="%d frames of %d x %d at %d spp, jitter_sequence(%d)" % (TQ.FRAMES, TQ.LW, TQ.LH, TQ.SPP, TQ.FRAMES),
               hi="%d x %d" % (TQ.W, TQ.H), max_history=TQ.MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN,
               rms_b_last_frame_upsampled=b, rms_c_accumulated_lo_upsampled=c,
               best=dict(best, ratio_a_over_b=best["rms"] / b, ratio_a_over_c=best["rms"] / c), sweep=rows)
    with open(os.path.join(ROOT, "profiles", "temporal_upsample", "quality.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "sweep"}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
