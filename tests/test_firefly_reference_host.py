"""art_firefly_device without a GPU: the product's per-pixel text (csrc/art_firefly.h) compiled by g++ with AddressSanitizer and UBSan
against the numpy reference written from the header (tests/firefly_ref.py), bit for bit on every output word, moments word and flag
byte, on the synthetic cases the GPU test shares; the stand-alone program's own checks; what the cases cover; and one frame by hand.

THE CASE BY HAND.  A 3 x 3 frame, green channel only, every value a power of two, scale 1, so that with a = 0.7152f every luminance
l = (0.2126f * 0 + 0.7152f * g) + 0.0722f * 0 = a * g is exact.  Green, and the moments (S1, S2) = (g, g * g) of one colour:

      1   2   1
      4  64   2          radius 1, rank 2, gain 2, floor 0, min_count 2, no id
      1   8   1

Centre: its eight neighbours hold the keys a * {1, 2, 1, 4, 2, 1, 8, 1}; the largest is 8 a, the second largest m = 4 a;
T = amax(2 * 4 a + 0, 0) = 8 a (a doubling is exact);  l = 64 a > 8 a;  f = 8 a / 64 a = 0.125 exactly (the quotient of two numbers
with the same significand is a power of two).  out = 0.125 * (0, 64, 0) = (0, 8, 0) = the words 0x00000000 0x41000000 0x00000000;
moments_out = (0.125 * 64, (0.125 * 0.125) * 4096) = (8, 64) = 0x41000000 0x42800000;  flag 1.
Every other pixel is kept with flag 0, e.g. the 8 below the centre: its five neighbours hold a * {4, 64, 2, 1, 1}, m = 4 a, T = 8 a,
and 8 a > 8 a is false; the 4 to the left: a * {1, 2, 64, 1, 8}, m = 8 a, T = 16 a.  With rank 1 the centre has m = 8 a, T = 16 a,
f = 0.25: out = (0, 16, 0), moments_out = (16, 256)."""
import subprocess

import numpy as np
import pytest

import firefly_ref as R

F = np.float32
U32 = np.uint32


def test_program_checks_itself():
    out = subprocess.check_output([R.host_program()], text=True)
    assert "firefly_host: ok" in out


def by_hand():
    green = np.array([[1, 2, 1], [4, 64, 2], [1, 8, 1]], F)
    color = np.zeros((3, 3, 3), F)
    color[..., 1] = green
    return color, np.stack([green, green * green], -1)


@pytest.mark.parametrize("run", [R.firefly, R.firefly_host], ids=["reference", "host"])
def test_the_case_by_hand(run):
    color, moments = by_hand()
    out, mo, flag = run(color, moments, radius=1, rank=2, gain=2.0, floor=0.0, min_count=2)
    want, wm = color.copy(), moments.copy()
    want[1, 1, 1] = 8.0
    wm[1, 1] = (8.0, 64.0)
    assert R.differ(out, want) == 0 and R.differ(mo, wm) == 0 and flag.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert out.view(U32)[1, 1].tolist() == [0, 0x41000000, 0] and mo.view(U32)[1, 1].tolist() == [0x41000000, 0x42800000]
    out, mo, flag = run(color, moments, radius=1, rank=1, gain=2.0)
    assert out[1, 1].tolist() == [0.0, 16.0, 0.0] and mo[1, 1].tolist() == [16.0, 256.0] and int(flag.sum()) == 1


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_build_equals_the_reference(size):
    W, H = size
    for name, kw in R.cases(W, H):
        ref = R.firefly(**kw)
        assert R.differ_all(R.firefly_host(**kw), ref) == 0, name
        assert R.differ_all(R.firefly_host(in_place=True, **kw), ref) == 0, name + " (in place)"


def test_in_place_in_the_references_terms():
    """the reference never writes its inputs; handing its result back as the input of a second call is what a caller who works in place
    does next: the second call sees the clamped frame (scale 1 now), and a frame clamped at gain 1, rank 1 is a fixed point of neither
    -- but every value can only go down, and nothing that was kept and whose neighbours were kept changes"""
    color, moments, ids = R.frame(33, 19)
    a = R.firefly(color, moments, ids, radius=2, rank=2, gain=2.0, scale=0.25)
    b = R.firefly(a[0], a[1], ids, radius=2, rank=2, gain=2.0, scale=1.0)
    assert (R.lum3(b[0]) <= R.lum3(a[0])).all() and (a[2] == 1).any()
    keep = np.ones((19, 33), bool)
    for y, x in zip(*np.nonzero(a[2])):
        keep[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = False
    assert keep.any() and R.differ(b[0][keep], a[0][keep]) == 0 and not b[2][keep].any()


def test_the_cases_cover_what_they_name():
    """the inputs do what their names say, on the reference's own outputs"""
    W, H = 33, 19
    cs = dict(R.cases(W, H))
    for radius in R.RADII:
        n = {1: 8, 2: 24}[radius]
        out, mo, flag = R.firefly(**cs["r%d rank 1" % radius])
        assert 0 < (flag == 1).sum() < W * H and not (flag == 2).any() and np.isfinite(out).all() and np.isfinite(mo).all()
        kw = cs["r%d rank 2" % radius]
        one, two = R.firefly(**dict(kw, rank=1))[2], R.firefly(**kw)[2]
        assert ((two == 1) & (one == 0)).any()                    # of two spikes side by side rank 1 takes the larger, rank 2 both
        # min_count at its upper end: only pixels with a full window can be clamped, so nothing within `radius` of the border is
        flag = R.firefly(**cs["r%d min_count full" % radius])[2]
        inner = np.zeros((H, W), bool); inner[radius:H - radius, radius:W - radius] = True
        assert kw["color"].shape == (H, W, 3) and (flag[inner] == 1).any() and not flag[~inner].any() and n == (2 * radius + 1) ** 2 - 1
        # planted bad values: flag 2 exactly where a channel of scale * colour is not finite; every NaN word is the quiet NaN; negative
        # channels are not bad; the words of bad pixels' moments are copied
        kw = cs["r%d planted bad" % radius]
        out, mo, flag = R.firefly(**kw)
        with np.errstate(all="ignore"):
            c = (F(kw["scale"]) * kw["color"]).astype(F)
        bad = ~np.isfinite(c).all(-1) | ~np.isfinite(R.lum3(c))
        assert bad.sum() >= 6 and ((flag == 2) == bad).all() and (kw["color"] < 0).any()
        assert (out.view(U32)[np.isnan(out)] == 0x7fc00000).all() and (kw["color"].view(U32)[np.isnan(kw["color"])] != 0x7fc00000).any()
        assert R.differ(mo[flag != 1], kw["moments"][flag != 1]) == 0
        assert np.isfinite(out[~bad]).all()                       # no finite input produces a non-finite output
        # ties and black
        out, mo, flag = R.firefly(**cs["r%d equal keys" % radius])
        assert not flag.any() and R.differ(out, cs["r%d equal keys" % radius]["color"]) == 0
        out, mo, flag = R.firefly(**cs["r%d black, floor 0" % radius])
        assert not flag.any() and not out.any() and not mo.any()
        out, mo, flag = R.firefly(**cs["r%d huge gain" % radius])
        assert np.isfinite(out).all() and (flag == 1).any()      # gain * m overflows to -infinity under negative keys: T = 0, the pixel goes to 0
    # with ids fewer pixels have a full window: the ids are bands five columns wide, so a pixel in a band's first or last column is kept
    kw = cs["r1 min_count full, ids"]
    with_ids, without = R.firefly(**kw)[2], R.firefly(**dict(kw, ids=None))[2]
    edge = np.isin(np.arange(W) % 5, (0, 4))
    assert with_ids.any() and not with_ids[:, edge].any() and without[:, edge].any()
