"""The point of the variance-guided denoiser, on the CPU: with the shipped defaults of Backend.denoise_svgf_torch the numpy reference
brings the RMS error of the 8-spp test frame below the unfiltered frame's (profiles/svgf/quality.json: the sweep found settings that do so
at 4, 8 and 16 spp and these are the best of them)."""
import json
import os

import numpy as np

import svgf_quality as Q
import svgf_ref as S


def test_shipped_defaults_are_the_sweeps_best(art):
    q = json.load(open(os.path.join(art.ROOT, "profiles", "svgf", "quality.json")))
    assert q["svgf_improves_at_every_spp"] and set(q["best_svgf"]["spp"]) == {"4", "8", "16"}
    assert (q["best_svgf"]["sigma_color"], q["best_svgf"]["iterations"]) == (art.SVGF_SIGMA_COLOR, art.SVGF_ITERATIONS)
    import inspect
    d = inspect.signature(art.Backend.denoise_svgf_torch).parameters
    assert d["sigma_color"].default == art.SVGF_SIGMA_COLOR and d["iterations"].default == art.SVGF_ITERATIONS


def test_filtered_8_spp_is_closer_to_the_reference_than_unfiltered(art):
    ref = Q.reference()
    acc, mom, guides = Q.cpu_inputs(art)
    before = Q.rms(acc / np.float32(Q.SPP), ref)
    out, _ = S.denoise(acc, mom, Q.SPP, **guides, iterations=art.SVGF_ITERATIONS, sigma_color=art.SVGF_SIGMA_COLOR, scale=1.0 / Q.SPP)
    after = Q.rms(out, ref)
    print("RMS against 1024 spp: %.4f before, %.4f after" % (before, after))
    assert after < before
