"""The variance-guided denoiser and the luminance moments without a GPU: the product's per-pixel text (csrc/art_denoise.h svgf_*,
csrc/art_shade.h accumulate_pixel_moments) compiled by g++ against the two numpy references written from the header comments
(tests/svgf_ref.py, tests/moments_ref.py), bit for bit; accumulate_pixel_moments' accum against accumulate_pixel's; exact properties."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import moments_ref as M
import orc
import svgf_ref as S

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_build_equals_the_numpy_reference(size):
    W, H = size
    pl = R.planes(W, H)
    for c in S.combos():
        color, mom, nc, g, kw = S.combo_args(pl, c, W, H)
        got, want = S.denoise_host(color, mom, nc, **g, **kw), S.denoise(color, mom, nc, **g, **kw)
        assert S.differ(got[0], want[0]) == 0 and S.differ(got[1], want[1]) == 0, S.combo_id(c)


def test_non_finite_inputs_are_repaired_and_not_spread():
    """a NaN colour, an infinite moment (no colour stop at that centre), a NaN depth and a NaN normal: host build = reference; the colour
    is finite everywhere after the first iteration that reaches a good neighbour; the variance is never negative or NaN"""
    W, H = 37, 23
    color, albedo, normal, depth = [x.copy() for x in R.planes(W, H)]
    mom = S.moments_for(color, 4, W, H)
    color[9, 20] = np.nan; color[20, 30, 1] = np.inf
    mom[9, 9, 1] = np.inf; mom[10, 3] = np.nan; mom[2, 30, 0] = -np.inf
    depth[12, 20] = np.nan; normal[15, 5, 0] = np.nan
    for it in (1, 3):
        kw = dict(albedo=albedo, normal=normal, depth=depth, iterations=it, scale=0.25)
        got, want = S.denoise_host(color, mom, 4, **kw), S.denoise(color, mom, 4, **kw)
        assert S.differ(got[0], want[0]) == 0 and S.differ(got[1], want[1]) == 0
        assert np.isfinite(want[0]).all() and (want[1] >= 0).all()
    # not spread: a pixel more than 2 taps away from every broken one is what it is without them (one iteration)
    clean = R.planes(W, H)
    a = S.denoise(clean[0], S.moments_for(clean[0], 4, W, H), 4, albedo=albedo, normal=clean[2], depth=clean[3], iterations=1, scale=0.25)[0]
    b = S.denoise(color, mom, 4, albedo=albedo, normal=normal, depth=depth, iterations=1, scale=0.25)[0]
    far = np.ones((H, W), bool)
    for (y, x) in ((9, 20), (20, 30), (9, 9), (10, 3), (2, 30), (12, 20), (15, 5)):
        far[max(0, y - 3):y + 4, max(0, x - 3):x + 4] = False
    assert far.sum() > 200 and np.array_equal(bits(a)[far], bits(b)[far])


def test_variance_of_a_constant_image():
    """equal colours, S2 = S1^2 / n exactly representable: v_0 = 0, every colour weight is exp(0), the picture stays what it is and the
    variance stays 0; with a uniform v_0 > 0 and no guides the variance after one iteration is v_0 * sum(h^2) / sum(h)^2 in the interior"""
    W, H = 16, 12
    color = np.full((H, W, 3), 2.0, F)
    mom = np.zeros((H, W, 2), F); mom[..., 0] = 8.0; mom[..., 1] = 16.0            # n = 4 colours of luminance 2: S1 = 8, S2 = 16
    for fn in (S.denoise, S.denoise_host):
        out, v = fn(color, mom, 4, iterations=3, scale=0.25)
        assert np.array_equal(out, np.full((H, W, 3), 0.5, F)) and not v.any()
    mom[..., 1] = 20.0                                                              # D = 4, v_0 = 4 * 4/3 / 16 = 1/3
    out, v = S.denoise(color, mom, 4, iterations=1, scale=0.25)
    k = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    want = (1.0 / 3.0) * (np.outer(k, k) ** 2).sum()
    assert abs(float(v[6, 8]) - want) < 1e-6 and np.allclose(out, 0.5, atol=1e-6)


def test_params_are_refused_by_the_host_build():
    color, mom = np.ones((2, 2, 3), F), np.ones((2, 2, 2), F)
    for kw in (dict(iterations=0), dict(iterations=9), dict(normal_log2=11), dict(scale=np.inf), dict(sigma_color=np.nan)):
        with pytest.raises(RuntimeError):
            S.denoise_host(color, mom, 2, **kw)
    with pytest.raises(RuntimeError):
        S.denoise_host(color, mom, 1)


# ---- the moments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [True, False], ids=["aa", "noaa"])
def test_accumulate_with_moments_equals_the_reference_and_the_plain_accum(aa):
    """three batches of random per-sample radiance over a sharded pixel list, some of it not finite: the g++ build of
    accumulate_pixel_moments gives the numpy reference's moments and accumulate_pixel's accum, word for word; pixels outside the list stay +0"""
    rng = np.random.default_rng(5)
    npix, frame, samples = 53, 140, 8
    pm = rng.permutation(frame)[:npix].astype(np.uint32)
    bg = np.array([0.125, 0.5, 0.25], F)
    accum, mom = np.zeros((frame, 3), F), np.zeros((frame, 2), F)
    ra, rm = np.zeros((npix, 3), F), np.zeros((npix, 2), F)
    for b in range(3):
        rad = np.exp(rng.uniform(np.log(1e-4), np.log(1e3), (samples, npix, 3))).astype(F)
        rad[rng.random((samples, npix)) < 0.3] = 0.0
        if b == 1:
            rad[3, 7, 1] = np.nan; rad[0, 11, 2] = np.inf
        accum, mom, plain_new = S.accumulate_host(rad, aa, bg, accum, mom, pm)
        ra, rm = M.add_colours(M.colours(rad, aa, bg), ra, rm)
        assert S.differ(accum, plain_new) == 0                      # (plain_new started from this batch's input accum)
        assert S.differ(accum[pm], ra) == 0 and S.differ(mom[pm], rm) == 0, "batch %d" % b
    rest = np.ones(frame, bool); rest[pm] = False
    assert not bits(accum)[rest].any() and not bits(mom)[rest].any()
    assert np.isnan(mom[pm[7]]).all() and not np.isfinite(mom[pm[11]]).any()      # a non-finite colour poisons the pixel's moments
    assert np.isfinite(np.delete(mom[pm], [7, 11], axis=0)).all()


def test_moments_do_not_depend_on_the_batches():
    """the same 16 samples in one batch, in two sample chunks and in four: the same words"""
    rng = np.random.default_rng(6)
    npix = 31
    rad = rng.random((16, npix, 3)).astype(F)
    bg = np.zeros(3, F)
    for aa in (True, False):
        whole = S.accumulate_host(rad, aa, bg, np.zeros((npix, 3), F), np.zeros((npix, 2), F))
        for chunk in (8, 4):
            a, m = np.zeros((npix, 3), F), np.zeros((npix, 2), F)
            for s0 in range(0, 16, chunk):
                a, m, _ = S.accumulate_host(rad[s0:s0 + chunk], aa, bg, a, m)
            assert np.array_equal(bits(a), bits(whole[0])) and np.array_equal(bits(m), bits(whole[1]))


def test_moments_of_oracle_samples():
    """the oracle's per-sample radiance of the reference scene, 12 x 8, 8 samples with anti-aliasing: the reference's accum is the oracle's
    own two passes (so the colours are cut and ordered as a pass does), and the g++ build agrees with the reference's moments"""
    W, H = 12, 8
    cs = orc.CornellScene()
    prm = orc.make_params(W, H, orc.PT_MIS, True, 4, 1, seed=3)
    rad = M.sample_radiance(cs.scene, prm, 0, 8)
    cols = M.colours(rad, True)
    acc, mom = M.add_colours(cols)
    ref, spp, _ = orc.render(cs.scene, prm, passes=2)
    assert spp == 8 and np.array_equal(bits(acc), bits(ref)) and ref.any()
    a, m, _ = S.accumulate_host(rad.reshape(8, W * H, 3), True, np.zeros(3, F), np.zeros((W * H, 3), F), np.zeros((W * H, 2), F))
    assert np.array_equal(bits(a), bits(ref).reshape(-1, 3)) and np.array_equal(bits(m), bits(mom).reshape(-1, 2))
    n = 2
    D = mom[..., 1].astype(np.float64) - mom[..., 0].astype(np.float64) ** 2 / n
    assert (D > 0).mean() > 0.3                                      # the scene is noisy at this sample count: the moments say so


def test_the_stand_alone_program_runs_clean():
    """tests/svgf_host/svgf_host: the same functions behind a main of their own (the target of the sanitizer build, `make svgf_host_san`)"""
    d = os.path.join(S.HERE, "svgf_host")
    subprocess.check_call(["make", "-s", "-C", d, "svgf_host"])
    out = subprocess.run([os.path.join(d, "svgf_host")], capture_output=True, text=True)
    assert out.returncode == 0 and "svgf_host: ok" in out.stdout, out.stdout + out.stderr
