"""art_upsample_device without a GPU: the product's text (csrc/art_upsample.h) compiled by g++ as a stand-alone program (with
AddressSanitizer and UBSan) against the numpy reference written from the header (tests/upsample_ref.py), bit for bit on every out3f word
and every fallback1b byte of the shapes and cases the GPU test shares; the program's own checks; and the properties that follow from the
arithmetic, each written as a function of "an upsampler" so that tests/test_gpu_upsample.py asserts them of the kernels too."""
import subprocess

import numpy as np
import pytest

import upsample_ref as U

F = np.float32


def test_program_checks_itself():
    out = subprocess.check_output([U.host_program()], text=True)
    assert "upsample_host: ok" in out


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_host_build_equals_the_reference(shape):
    refs = U.reference_results(shape)
    got = U.upsample_host_many([kw for _, kw, _ in refs])
    for (name, kw, (out, fb)), (hout, hfb) in zip(refs, got):
        assert U.differ(out, hout) == 0, name + ": out3f"
        assert U.differ(fb, hfb) == 0, name + ": fallback1b"
        assert np.isfinite(out).all(), name + ": a value that is not finite"


def test_the_cases_cover_what_they_name():
    """the planted frames hold what planes() says, and the reference's fallback bytes show every kind of pixel on them"""
    for shape in U.SHAPES:
        W, H, LW, LH, _ = shape
        lo_color, lo, hi = U.planes(W, H, LW, LH)
        res = {name: r for name, _, r in U.reference_results(shape)}
        assert len(res) == 22
        if LW * LH < 15:
            assert all(fb.max() <= 1 for _, fb in res.values()) and (res["fp2_none"][1] == 0).all()      # (nothing is planted on a lo frame this small)
            continue
        assert np.isnan(lo_color).any() and np.isinf(lo_color).any() and (lo_color < 0).any()
        assert all(not np.isfinite(g[k]).all() for g in (lo, hi) for k in ("albedo", "normal", "depth"))
        assert (hi["normal"] == 0).all(axis=-1).any() and (lo["normal"] == 0).all(axis=-1).any() and (lo["depth"] < 0).any() and (hi["depth"] < 0).any()
        assert len(np.unique(lo["id"])) >= 2 and (hi["id"] == U.ID_ALONE).sum() == 1 and not (lo["id"] == U.ID_ALONE).any()
        for fp in (2, 4):
            for name in ("none", "all_demod", "id"):
                assert res["fp%d_%s" % (fp, name)][1][0, 0] == 2, (shape, fp, name)        # every tap of the corner pixel is clamped into the block without a colour
            alone = tuple(np.argwhere(hi["id"] == U.ID_ALONE)[0])
            assert res["fp%d_id" % fp][1][alone] == 1 and res["fp%d_all_demod" % fp][1][alone] == 1
            assert (res["fp%d_all_demod" % fp][1] == 0).mean() > 0.5
            assert res["fp%d_none" % fp][1].max() == 2 and not (res["fp%d_none" % fp][1] == 1).any()      # without guides nothing can fall back to "unguided"


# ---- the properties, of any upsampler with upsample_ref.upsample's signature ------------------------------------------------------------
def bilinear(lo_color, W, H, jitter=(0.0, 0.0)):
    """an independent plain bilinear interpolation of a finite lo plane: the header's mapping in binary32 (the coordinates are part of
    the contract), the interpolation itself in binary64 with its own index arithmetic"""
    LH, LW = lo_color.shape[:2]
    c = np.asarray(lo_color, np.float64)
    u = ((np.arange(W).astype(F) + F(0.5)) * (F(LW) / F(W)) - (F(0.5) + F(jitter[0]))).astype(np.float64)
    v = ((np.arange(H).astype(F) + F(0.5)) * (F(LH) / F(H)) - (F(0.5) + F(jitter[1]))).astype(np.float64)
    x0, y0 = np.floor(u).astype(int), np.floor(v).astype(int)
    tx, ty = (u - x0)[None, :, None], (v - y0)[:, None, None]
    X0, X1, Y0, Y1 = np.clip(x0, 0, LW - 1), np.clip(x0 + 1, 0, LW - 1), np.clip(y0, 0, LH - 1), np.clip(y0 + 1, 0, LH - 1)
    top = c[Y0][:, X0] * (1 - tx) + c[Y0][:, X1] * tx
    bot = c[Y1][:, X0] * (1 - tx) + c[Y1][:, X1] * tx
    return top * (1 - ty) + bot * ty


def no_guides_is_bilinear(run, shape):
    """with no guide the output is the plain bilinear interpolation to 1e-6 relative: the colours are positive, so the result is a sum of
    positive terms and each of the product's binary32 roundings (two weights, their product, four products with the colour and the scale,
    six sums, one division: under sixteen of 2^-24 each) moves it by at most that share of itself"""
    W, H, LW, LH, jitter = shape
    lo_color, _, _ = U.clean_planes(W, H, LW, LH)
    out, fb = run(lo_color=lo_color, size=(W, H), footprint=2, jitter=jitter, demodulate=False)
    want = bilinear(lo_color, W, H, jitter)
    assert (fb == 0).all() and (lo_color > 0).all()
    assert (np.abs(out - want) <= 1e-6 * want).all(), float((np.abs(out - want) / want).max())


def id_boundary_keeps_the_sides_apart(run, shape, names=("id",)):
    """two constant colours either side of the id boundary: a hi pixel with any tap of its own id takes no colour from the other side, so it
    equals its side's colour to 1e-6 relative (a weighted mean of equal values: one rounding per product, sum and the division); a hi
    pixel with none is flagged 1"""
    W, H, LW, LH, jitter = shape
    _, lo, hi = U.clean_planes(W, H, LW, LH)
    colours = {U.ID_A: np.array([4.0, 0.5, 0.25], F), U.ID_B: np.array([0.125, 2.0, 8.0], F), U.ID_MISS: np.array([1.0, 1.0, 1.0], F)}
    lo_color = np.zeros((LH, LW, 3), F)
    for ident, c in colours.items():
        lo_color[lo["id"] == ident] = c
    i0, _, _ = U.axis(W, LW, jitter[0])
    j0, _, _ = U.axis(H, LH, jitter[1])
    for fp in (2, 4):
        out, fb = run(lo_color=lo_color, lo=U.subset(lo, names), hi=U.subset(hi, names), footprint=fp, jitter=jitter, demodulate=False, sigma_depth=1.0, normal_log2=5)
        same = np.zeros((H, W), bool)
        for b in U.taps(fp):
            for a in U.taps(fp):
                same |= lo["id"][np.clip(j0 + b, 0, LH - 1)[:, None], np.clip(i0 + a, 0, LW - 1)[None, :]] == hi["id"]
        want = np.stack([np.where(hi["id"] == U.ID_A, colours[U.ID_A][k], np.where(hi["id"] == U.ID_B, colours[U.ID_B][k], F(1))) for k in range(3)], axis=-1)
        ok = same & (fb == 0)
        assert ok.sum() > 0 and (np.abs(out - want)[ok] <= 1e-6 * want[ok]).all(), (shape, fp)
        assert (fb[~same] == 1).all(), (shape, fp)
        if names == ("id",):
            assert (fb[same] == 0).all(), (shape, fp)


def background_is_not_flagged(run, shape):
    """with every guide, a background hi pixel (zero normal) one of whose 2 x 2 lo taps is background too is reconstructed from them:
    fallback 0 -- without the rule its normal weight would be 0 for every tap"""
    W, H, LW, LH, jitter = shape
    lo_color, lo, hi = U.clean_planes(W, H, LW, LH)
    i0, fx, _ = U.axis(W, LW, jitter[0])
    j0, fy, _ = U.axis(H, LH, jitter[1])
    miss_lo, miss_hi = (lo["normal"] == 0).all(axis=-1), (hi["normal"] == 0).all(axis=-1)
    for fp in (2, 4):
        out, fb = run(lo_color=lo_color, lo=lo, hi=hi, footprint=fp, jitter=jitter, demodulate=True, sigma_depth=1.0, normal_log2=5)
        near = np.zeros((H, W), bool)                      # the nearest lo pixel, whose weight is not 0 under either footprint
        near |= miss_lo[np.clip(j0 + (fy >= 0.5), 0, LH - 1)[:, None], np.clip(i0 + (fx >= 0.5), 0, LW - 1)[None, :]]
        sel = miss_hi & near
        assert sel.sum() > 0 and (fb[sel] == 0).all(), (shape, fp)
        assert (fb[~miss_hi & ~near] <= 1).all()


PROPERTY_SHAPES = [s for s in U.SHAPES if s[2] * s[3] >= 15]


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_no_guides_is_bilinear(shape):
    no_guides_is_bilinear(U.upsample, shape)
    no_guides_is_bilinear(U.upsample_host, shape)


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=U.SHAPE_IDS)
def test_id_boundary_keeps_the_sides_apart(shape):
    for run in (U.upsample, U.upsample_host):
        id_boundary_keeps_the_sides_apart(run, shape)
        id_boundary_keeps_the_sides_apart(run, shape, U.GUIDES)


@pytest.mark.parametrize("shape", PROPERTY_SHAPES[1:], ids=U.SHAPE_IDS)
def test_background_is_not_flagged(shape):
    background_is_not_flagged(U.upsample, shape)
    background_is_not_flagged(U.upsample_host, shape)
