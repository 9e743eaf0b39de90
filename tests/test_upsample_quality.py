"""Guided upsampling against plain interpolation on the 48 x 48 test scene, without a GPU: the numpy reference on the oracle's samples
(tests/upsample_quality.py) with the setting the sweep shipped (profiles/upsample/quality.json, whose sigma_depth and normal_log2 are
upsample_torch's defaults).  The sweep measured r = rms(guided) / rms(unguided) = 0.235; the assertion is guided < ((1 + r) / 2) *
unguided, halfway between the measured ratio and no gain.  The same ray budget spent at full resolution (48 x 48 at 4 spp) is printed
beside both and not asserted against."""
import numpy as np

import upsample_quality as UQ
import upsample_ref as U

_inputs = None


def inputs(art):
    """(lo colour, lo guides, hi guides) from the oracle, once per process (tests/test_gpu_upsample.py shares them)"""
    global _inputs
    if _inputs is None:
        lo_color, lo = UQ.cpu_frame(art, UQ.LW, UQ.LH, UQ.LO_SPP)
        _, hi = UQ.cpu_frame(art, UQ.W, UQ.H, 0)
        _inputs = (lo_color, lo, hi)
    return _inputs


def best_call(lo, hi):
    """the shipped setting as keyword arguments of upsample_ref.upsample / upsample_torch's runner, and the bound it is held to"""
    rec = UQ.record()
    b = rec["best"]
    names = ("albedo", "normal", "depth") + (("id",) if b["ids"] else ())
    assert b["ratio"] < 1.0 and abs(b["ratio"] - b["rms"] / rec["rms_unguided"]) < 1e-12
    return dict(lo=U.subset(lo, names), hi=U.subset(hi, names), footprint=b["footprint"], sigma_depth=b["sigma_depth"], normal_log2=b["normal_log2"],
                demodulate=b["demodulate"]), 0.5 * (1.0 + b["ratio"]), rec


def guided_beats_unguided(run, art):
    """of any upsampler with upsample_ref.upsample's signature"""
    lo_color, lo, hi = inputs(art)
    kw, bound, rec = best_call(lo, hi)
    ref = UQ.reference().astype(np.float64)
    guided = UQ.rms(run(lo_color=lo_color, **kw)[0], ref)
    unguided = UQ.rms(run(lo_color=lo_color, size=(UQ.W, UQ.H), footprint=2, demodulate=False)[0], ref)
    print("rms against the 1024-spp picture: guided %.6f, unguided %.6f (ratio %.4f, bound %.4f); 48 x 48 at 4 spp: %.6f (recorded)"
          % (guided, unguided, guided / unguided, bound, rec["rms_same_budget_full_resolution"]))
    assert guided < bound * unguided


def test_guided_upsampling_beats_plain_interpolation(art):
    guided_beats_unguided(U.upsample, art)


def test_the_defaults_are_the_swept_setting(art):
    b = UQ.record()["best"]
    assert (art.upsample.UPSAMPLE_SIGMA_DEPTH, art.upsample.UPSAMPLE_NORMAL_LOG2) == (b["sigma_depth"], b["normal_log2"])
