"""Inputs of the quality tests of adaptive sampling: the scene and the 1024-spp reference picture of profiles/svgf and profiles/temporal
(scenes.synthetic_scene(2000, 3), 48 x 48, PT_MIS, depth 8, no anti-aliasing, seed 7; tests/golden/svgf_quality_ref_48x48.npy, the CPU
oracle's own estimator, seed 11 -- the anti-aliasing setting is the same, so no new golden), the budget and the loop's shape, and the
figure: RMS against the reference of the adaptive loop's mean picture and of uniform sampling with the WHOLE budget (the loop stops before
the pass that would exceed the budget, so uniform never has fewer samples than adaptive)."""
import json
import os

import numpy as np

import svgf_quality as SQ

F = np.float32
W, H, SEED, DEPTH = SQ.W, SQ.H, SQ.SEED, SQ.DEPTH
AA = False
BUDGET_SPP = 32                      # the budget: this many samples per pixel on average
BUDGET = BUDGET_SPP * W * H
FIRST_VTHREADS = 4                   # the full pass: 4 samples everywhere
STEP_VTHREADS = 4                    # every masked pass: 4 more samples where the mask says so
MAX_SAMPLES = 256                    # no pixel takes more (the oracle's samples are computed up to here)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

reference = SQ.reference
rms = SQ.rms
scene = SQ.scene


def shipped():
    """the sweep's record (profiles/adaptive/quality.json)"""
    with open(os.path.join(ROOT, "profiles", "adaptive", "quality.json")) as f:
        return json.load(f)


def bound(best):
    """the asserted ratio: halfway between 1 and what the CPU loop reached in the sweep"""
    return 0.5 * (1.0 + best["ratio"])


_rad = {}


def radiance(art):
    """the oracle's radiance of samples 0 .. MAX_SAMPLES - 1 of every pixel, [MAX_SAMPLES, H, W, 3]; computed once, read-only"""
    if "rad" not in _rad:
        import conv, hostsim, moments_ref, orc
        sd = scene()
        osc = conv.OracleScene(sd)
        nodes, tris, info = hostsim.bvh(art, sd)
        osc.attach_bvh(nodes, tris, info["width"])
        r = moments_ref.sample_radiance(osc.scene, orc.make_params(W, H, orc.PT_MIS, AA, DEPTH, 1, seed=SEED), 0, MAX_SAMPLES)
        r.setflags(write=False)
        _rad["rad"] = r
    return _rad["rad"]


def uniform_picture(rad):
    import moments_ref
    acc, _ = moments_ref.add_colours(moments_ref.colours(rad[:BUDGET_SPP], AA))
    return acc / F(BUDGET_SPP)


def adaptive_picture(rad, threshold, lum_floor, min_colours):
    """(mean picture, counts, passes) of the CPU loop (tests/adaptive_ref.adaptive_loop) with the budget and the loop's shape above"""
    import adaptive_ref
    acc, mom, counts, passes = adaptive_ref.adaptive_loop(rad, AA, BUDGET, STEP_VTHREADS, threshold, lum_floor, min_colours, MAX_SAMPLES, first_vthreads=FIRST_VTHREADS)
    mean = adaptive_ref.estimate(acc, mom, counts, AA, min_colours, MAX_SAMPLES, threshold, lum_floor)[0]
    return mean, counts, passes
