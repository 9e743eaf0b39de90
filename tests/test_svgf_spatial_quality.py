"""The spatial variance estimate lowers the error at one colour per frame (CPU): the second and the last of four oracle frames along a
pan, accumulated and filtered by the numpy references with the shipped defaults, WITH art_svgf_spatial_variance_device's reference
between the two and WITHOUT it (the chain as it was), against the oracle's 1024-spp pictures of those cameras.  The asserted ratios are
halfway between 1 and what the references reached in the sweep of profiles/svgf_spatial/quality.py."""
import numpy as np

import svgf_spatial_quality as Q


def test_shipped_defaults_are_the_sweeps_best(art):
    rec = Q.shipped()
    best = rec["best"]
    assert (art.SVGF_SPATIAL_RADIUS, art.SVGF_SPATIAL_MIN_HISTORY, art.SVGF_SPATIAL_SIGMA_DEPTH) == (best["radius"], best["min_history"], best["sigma_depth"])
    assert (art.SVGF_ITERATIONS, art.SVGF_SIGMA_COLOR) == (best["iterations"], best["sigma_color"])
    assert best["ratio_second"] < 1 and best["ratio_last"] < 1
    assert rec["asserted_ratio_second"] == Q.bound(best["ratio_second"]) and rec["asserted_ratio_last"] == Q.bound(best["ratio_last"])


def test_filtered_frames_are_closer_to_the_reference_with_the_call(art):
    rec = Q.shipped()
    frames = [Q.cpu_frame(art, k)[:3] for k in range(Q.FRAMES)]
    steps = Q.accumulate(art, frames)
    kw = dict(radius=art.SVGF_SPATIAL_RADIUS, min_history=art.SVGF_SPATIAL_MIN_HISTORY, sigma_depth=art.SVGF_SPATIAL_SIGMA_DEPTH)
    assert np.isinf(steps[0][1]).all()                       # one colour per frame: the first frame has no variance anywhere
    for name, k, ref in zip(("second", "last"), (Q.SECOND, Q.LAST), Q.reference()):
        with_, var = Q.filtered(steps[k], art.SVGF_ITERATIONS, art.SVGF_SIGMA_COLOR, kw)
        without = Q.filtered(steps[k], art.SVGF_ITERATIONS, art.SVGF_SIGMA_COLOR)[0]
        a, b = Q.rms(with_, ref), Q.rms(without, ref)
        print("%s frame: RMS against 1024 spp %.4f with the call, %.4f without; bound %.4f" % (name, a, b, rec["asserted_ratio_" + name]))
        assert a < rec["asserted_ratio_" + name] * b
        hit = steps[k][3]["depth"] > 0
        assert np.isfinite(var[hit]).mean() > np.isfinite(steps[k][1][hit]).mean()
