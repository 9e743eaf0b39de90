"""Temporal super-resolution against its two neighbours on the 48 x 48 test scene, without a GPU: the numpy references on the oracle's
samples (tests/temporal_upsample_quality.py) with the setting the sweep shipped (profiles/temporal_upsample/quality.json, whose radius and
min_confidence are temporal_upsample_torch's defaults).  After 8 jittered 24 x 24 frames at 4 spp the sweep measured
  A / B = rms(accumulated into 48 x 48) / rms(the last frame alone, guided upsampling)            = 0.142
  A / C = rms(accumulated into 48 x 48) / rms(8 unjittered frames accumulated at 24 x 24, upsampled) = 0.574
and both are asserted at the halfway bound, A < ((1 + r) / 2) * B: 0.571 and 0.787.  A / C below 1 says that on this scene putting the
samples where they were taken beats accumulating them on the lo grid."""
import numpy as np

import temporal_upsample_quality as TQ
import temporal_upsample_ref as R


def bounds():
    b = TQ.record()["best"]
    assert b["ratio_a_over_b"] < 1.0 and b["ratio_a_over_c"] < 1.0
    return b, 0.5 * (1.0 + b["ratio_a_over_b"]), 0.5 * (1.0 + b["ratio_a_over_c"])


def accumulation_beats_its_neighbours(run, art):
    """of any implementation with temporal_upsample_ref.temporal_upsample's signature"""
    b, bound_b, bound_c = bounds()
    ref = TQ.reference().astype(np.float64)
    a = TQ.rms(TQ.chain_a(run, art, b["radius"], b["min_confidence"], b["demodulate"]), ref)
    last, lo = TQ.rms(TQ.chain_b(art), ref), TQ.rms(TQ.chain_c(art), ref)
    print("rms against the 1024-spp picture: (A) %.6f, (B) %.6f, (C) %.6f: A / B %.4f (bound %.4f), A / C %.4f (bound %.4f)"
          % (a, last, lo, a / last, bound_b, a / lo, bound_c))
    assert a < bound_b * last
    assert a < bound_c * lo


def test_accumulated_jittered_frames_beat_one_frame_and_plain_accumulation(art):
    accumulation_beats_its_neighbours(R.temporal_upsample, art)


def test_the_record_is_the_sweeps(art):
    rec = TQ.record()
    b = rec["best"]
    assert b["rms"] == min(r["rms"] for r in rec["sweep"])
    assert abs(b["ratio_a_over_b"] - b["rms"] / rec["rms_b_last_frame_upsampled"]) < 1e-12
    assert abs(b["ratio_a_over_c"] - b["rms"] / rec["rms_c_accumulated_lo_upsampled"]) < 1e-12


def test_the_defaults_are_the_swept_setting(art):
    b = TQ.record()["best"]
    assert (art.temporal_upsample.TEMPORAL_UPSAMPLE_RADIUS, art.temporal_upsample.TEMPORAL_UPSAMPLE_MIN_CONFIDENCE) == (b["radius"], b["min_confidence"])
