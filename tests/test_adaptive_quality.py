"""Adaptive sampling lowers the error at an equal budget (CPU): the plain loop of Backend.render_adaptive, driven by the numpy reference of
the estimate over the CPU oracle's own samples (pixel q takes sample indices spp .. spp + S - 1 in the passes that select it), against
uniform sampling with the whole budget, both held to the oracle's 1024-spp picture.  The asserted ratio is halfway between 1 and what
the loop reached in the sweep of profiles/adaptive/quality.py."""
import adaptive_quality as Q


def test_shipped_defaults_are_the_sweeps_best(art):
    rec = Q.shipped()
    best = rec["best"]
    assert (art.ADAPTIVE_THRESHOLD, art.ADAPTIVE_LUM_FLOOR, art.ADAPTIVE_MIN_COLOURS) == (best["threshold"], best["lum_floor"], best["min_colours"])
    assert best["ratio"] < 1 and best["budget_spent"] and best["ratio"] == min(r["ratio"] for r in rec["rows"] if r["budget_spent"])
    assert abs(rec["asserted_ratio"] - Q.bound(best)) < 1e-12


def test_adaptive_is_closer_to_the_reference_than_uniform(art):
    rad, ref = Q.radiance(art), Q.reference()
    mean, counts, passes = Q.adaptive_picture(rad, art.ADAPTIVE_THRESHOLD, art.ADAPTIVE_LUM_FLOOR, art.ADAPTIVE_MIN_COLOURS)
    uniform, adaptive = Q.rms(Q.uniform_picture(rad), ref), Q.rms(mean, ref)
    best = Q.shipped()["best"]
    print("RMS against 1024 spp: uniform %d spp %.5f, adaptive %.5f with %d of %d samples in %d passes; bound %.3f"
          % (Q.BUDGET_SPP, uniform, adaptive, int(counts.sum()), Q.BUDGET, passes, Q.bound(best)))
    assert int(counts.sum()) <= Q.BUDGET and int(counts.max()) <= Q.MAX_SAMPLES
    assert adaptive < Q.bound(best) * uniform
