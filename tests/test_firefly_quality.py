"""Firefly suppression on the 48 x 48 test scene without a GPU: the numpy reference (tests/firefly_ref.py) on the oracle's samples
(tests/firefly_quality.py).

Planted spikes are the quality evidence: 12 pixels of the frame times 1000 must all be flagged and brought down, their neighbours and
everything else must come out as from the unplanted frame.

The sweep (profiles/firefly/quality.py -> quality.json) found NO setting that brings the accumulated history closer to the 1024-spp
picture on this scene: the best ratio (with the call / without) of the history's RMS at the last frame of the pan is 0.98 at 1 spp,
1.07 at 4 spp and 1.11 at 8 spp for the shipped setting (radius 2, rank 1, gain 8, floor 0.05), whose geometric mean over the three,
1.053, is the least of the sweep.  The frames hold no spike that is not light the picture really contains, so what the clamp removes
is bias.  What is asserted is therefore the price: the relative change of the last frame's mean luminance at 4 spp, measured -0.0211,
must stay within 1.5 times that, 0.0316."""
import numpy as np

import firefly_quality as FQ
import firefly_ref as R
import temporal_ref as T


def frames(art, spp=FQ.ASSERTED_SPP):
    return [FQ.cpu_frame(art, k, spp) for k in range(FQ.FRAMES)]


def test_planted_spikes_are_all_clamped_and_nothing_else_changes(art):
    acc, mom, _ = frames(art)[FQ.LAST]
    got = FQ.check_planted(R.firefly, acc, mom, 1.0 / FQ.ASSERTED_SPP)
    assert np.isfinite(got[0]).all()
    host = R.firefly_host(*FQ.plant(acc, mom, 1.0 / FQ.ASSERTED_SPP)[:2], None, scale=1.0 / FQ.ASSERTED_SPP, **FQ.PLANT_SETTING)
    assert R.differ_all(host, got) == 0


def price_of_the_clamp(art, firefly, temporal, fr, spp=FQ.ASSERTED_SPP):
    """of any implementation of the two calls over the pan's frames: the relative change of the last frame's mean luminance under the
    shipped setting is within the asserted bound; returns (the change, ratio_b)"""
    rec = FQ.record()
    ref = FQ.reference().astype(np.float64)
    base = FQ.chain(art, fr, spp, firefly, temporal)
    res = FQ.chain(art, fr, spp, firefly, temporal, FQ.shipped(art))
    change = FQ.mean_luminance(res[FQ.LAST][0]) / FQ.mean_luminance(base[FQ.LAST][0]) - 1.0
    ratio_b = FQ.rms(res[FQ.LAST][1], ref) / FQ.rms(base[FQ.LAST][1], ref)
    a = rec["asserted"]
    print("mean-luminance change of the last frame %.5f (measured %.5f, bound %.5f); history RMS with / without the call %.4f (measured %.4f, not asserted: no gain)"
          % (change, a["mean_luminance_change"], a["bound_mean_luminance_change"], ratio_b, a["ratio_b"]))
    assert a["spp"] == spp and a["bound_ratio_b"] is None            # the sweep found no gain: were there one, it would be asserted here
    assert abs(change) <= a["bound_mean_luminance_change"]
    return change, ratio_b


def test_the_price_of_the_clamp_stays_within_the_measured_bound(art):
    price_of_the_clamp(art, R.firefly, T.temporal, frames(art))


def test_the_defaults_are_the_swept_setting(art):
    rec = FQ.record()
    b, a = rec["best"], rec["asserted"]
    assert FQ.shipped(art) == {k: b[k] for k in ("radius", "rank", "gain", "floor", "ids")}
    assert b["geomean_ratio_b"] == min(r["geomean_ratio_b"] for r in rec["sweep"])
    at = b["per_spp"][str(a["spp"])]
    assert a["ratio_b"] == at["ratio_b"] >= 1.0 and a["bound_ratio_b"] is None
    assert a["bound_mean_luminance_change"] == 1.5 * abs(at["mean_luminance_change"])
