"""The denoiser without a GPU: the product's per-pixel text (csrc/art_denoise.h) compiled by g++ against the numpy reference written from
the header comment (tests/denoise_ref.py), bit for bit; exact properties of the filter; and the plain B3-spline case against binary64."""
import itertools
import math

import numpy as np
import pytest

import denoise_ref as R

F = np.float32


def test_exp_small_transcription_against_math_exp():
    """the reference's own exp_small: within 4 ulp of math.exp on a grid over its domain (math.exp itself is good to an ulp)"""
    t = np.concatenate([np.linspace(-200.0, 0.0, 20001), -np.logspace(-12, 2, 400), [-0.0]])
    got = R.exp_small(t)
    want = np.array([math.exp(v) for v in t])
    assert np.all(np.abs(got - want) <= 4 * np.spacing(want))


@pytest.mark.parametrize("W,H", R.SIZES, ids=["%dx%d" % s for s in R.SIZES])
def test_host_build_equals_the_reference_bit_for_bit(W, H):
    """192 parameter sets per size: iterations 1 / 2 / 5 x every subset of the guides x demodulate x sigma_color 0 / 4 x normal_log2 0 / 7.
    With 5 iterations on 37 x 23 the last iteration's taps (s = 16, reach 32) fall outside the image for some centres."""
    pl = R.planes(W, H)
    for c in R.combos():
        color, g, kw = R.combo_args(pl, c)
        assert R.differ(R.denoise_host(color, **g, **kw), R.denoise(color, **g, **kw)) == 0, R.combo_id(c)


def test_far_taps_fall_outside_the_image():
    """8 iterations on 37 x 23: from s = 32 on every tap but the centre is off-image; host build and reference agree"""
    color, albedo, normal, depth = R.planes(37, 23)
    kw = dict(albedo=albedo, normal=normal, depth=depth, iterations=8, scale=0.25)
    assert R.differ(R.denoise_host(color, **kw), R.denoise(color, **kw)) == 0


def test_an_all_zero_image_stays_all_zero():
    _, albedo, normal, depth = R.planes(7, 5)
    out = R.denoise(np.zeros((5, 7, 3), F), albedo, normal, depth, iterations=3)
    assert not out.view(np.uint32).any()


@pytest.mark.parametrize("normal_log2", [1, 7])
def test_normals_stop_the_filter(normal_log2):
    """two half-images with orthogonal normals: changing the colours of one half leaves every output word of the other unchanged"""
    W, H = 12, 6
    color, albedo, _, depth = R.planes(W, H)
    normal = np.zeros((H, W, 3), F); normal[:, :6] = (0, 0, 1); normal[:, 6:] = (1, 0, 0)
    other = color.copy(); other[:, 6:] = other[:, 6:] * F(3.0) + F(1.0)
    kw = dict(albedo=albedo, normal=normal, depth=depth, iterations=3, normal_log2=normal_log2)
    a, b = R.denoise(color, **kw), R.denoise(other, **kw)
    assert np.array_equal(a[:, :6].view(np.uint32), b[:, :6].view(np.uint32))
    assert not np.array_equal(a[:, 6:].view(np.uint32), b[:, 6:].view(np.uint32))


def test_a_nan_pixel_is_repaired_and_does_not_spread():
    W, H = 15, 11
    color, albedo, normal, depth = R.planes(W, H)
    normal[:] = (0, 0, 1)                                   # (no zero-normal block: every pixel has good neighbours)
    bad = color.copy(); bad[5, 7] = (np.nan, 1.0, 1.0)
    kw = dict(albedo=albedo, normal=normal, depth=depth, sigma_color=0.0)
    for it in (1, 3):
        assert np.isfinite(R.denoise(bad, iterations=it, **kw)).all()
    a, b = R.denoise(color, iterations=1, **kw), R.denoise(bad, iterations=1, **kw)
    yy, xx = np.mgrid[0:H, 0:W]
    untouched = (np.abs(yy - 5) > 2) | (np.abs(xx - 7) > 2)          # centres whose 5 x 5 taps (s = 1) do not include the NaN pixel
    assert np.array_equal(a[untouched].view(np.uint32), b[untouched].view(np.uint32))
    assert R.differ(R.denoise_host(bad, iterations=3, **kw), R.denoise(bad, iterations=3, **kw)) == 0


def test_a_pixel_whose_every_tap_is_skipped_keeps_its_value():
    one = np.full((1, 1, 3), np.nan, F); one[0, 0, 1] = 2.0
    for fn in (R.denoise, R.denoise_host):
        out = fn(one, iterations=2, demodulate=False)
        assert np.isnan(out[0, 0, 0]) and np.isnan(out[0, 0, 2]) and out[0, 0, 1] == F(2.0)


@pytest.mark.parametrize("iterations", [1, 3])
def test_plain_spline_blur_against_binary64(iterations):
    """No guides and sigma_color 0: every tap inside the image has w = h exactly (e = exp_small(-0) = 1), so an iteration is the B3-spline
    blur renormalised at the border.  The bound, derived and not measured (u = 2^-24, colours >= 0 so nothing cancels, nothing here is
    subnormal): wsum is a sum of multiples of 2^-8 not above 1 and so exact; each product w * c is off by a factor (1 + d), |d| <= u, and
    goes through at most 24 additions of the running sum, each another such factor, so acc = exact * (1 + d)^25 at worst; the division
    is one more: 26 factors, relative error gamma_26 = 26 u / (1 - 26 u) per iteration against the exact blur of the same input.  The blur
    is linear with non-negative weights, so the relative error of its input passes through unchanged and n iterations compound to
    (1 + gamma_26)^n - 1.  (scale = 1 is exact; the binary64 side's own error, about 30 * 2^-53, is far below.)"""
    W, H = 37, 23
    color = R.planes(W, H)[0]
    k = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    c = color.astype(np.float64)
    for i in range(iterations):
        s = 1 << i
        acc, ws = np.zeros_like(c), np.zeros((H, W))
        for dy, dx in itertools.product(range(-2, 3), range(-2, 3)):
            cq, inside = R._shift(c, s * dx, s * dy)
            acc += (k[dx + 2] * k[dy + 2]) * cq * inside[..., None]
            ws += (k[dx + 2] * k[dy + 2]) * inside
        c = acc / ws[..., None]
    u = 2.0 ** -24
    bound = (1.0 + 26 * u / (1 - 26 * u)) ** iterations - 1.0
    for fn in (R.denoise, R.denoise_host):
        got = fn(color, iterations=iterations, sigma_color=0.0, scale=1.0).astype(np.float64)
        assert np.all(np.abs(got - c) <= bound * c)
