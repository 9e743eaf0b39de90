"""Temporal accumulation lowers the error (CPU): the last of four oracle frames along a pan, accumulated and filtered by the numpy
references with the shipped defaults, against the oracle's 1024-spp picture of that camera.  The asserted ratio is halfway between 1
and what the references reached in the sweep of profiles/temporal/quality.py (the margin covers other samples than the sweep's)."""
import temporal_quality as Q


def test_shipped_defaults_are_the_sweeps_best(art):
    best = Q.shipped()
    assert (art.TEMPORAL_MAX_HISTORY, art.TEMPORAL_DEPTH_TOL, art.TEMPORAL_NORMAL_MIN) == (best["max_history"], best["depth_tol"], best["normal_min"])
    assert best["ratio_filtered"] < 1 and best["ratio_accumulated"] < 1


def test_accumulated_and_filtered_frame_is_closer_to_the_reference(art):
    frames = [Q.cpu_frame(art, k)[:3] for k in range(Q.FRAMES)]
    alone, acc, filt = Q.chain(frames, art.TEMPORAL_MAX_HISTORY, art.TEMPORAL_DEPTH_TOL, art.TEMPORAL_NORMAL_MIN, art.SVGF_ITERATIONS, art.SVGF_SIGMA_COLOR)
    ref = Q.reference()
    before, mid, after = Q.rms(alone, ref), Q.rms(acc, ref), Q.rms(filt, ref)
    print("RMS against 1024 spp: %.4f last frame alone, %.4f accumulated, %.4f accumulated and filtered; bound %.3f" % (before, mid, after, Q.bound(Q.shipped())))
    assert after < Q.bound(Q.shipped()) * before and mid < before
