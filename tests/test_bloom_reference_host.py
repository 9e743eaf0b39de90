"""art_bloom_device without a GPU: the product's per-texel text (csrc/art_bloom.h) compiled by g++ with AddressSanitizer and UBSan against
the numpy reference written from the header (tests/bloom_ref.py), bit for bit on every word of out3f, of bloom3f and of every pyramid
level after the down sweep and after the up sweep, on the synthetic cases the GPU test shares; the stand-alone program's own checks;
what the cases cover; one frame by hand; and the properties the header names (tests/test_gpu_bloom.py asserts them again on the GPU).

THE CASE BY HAND.  A 2 x 2 frame, red only: 8 0 / 0 0, scale 1, one level, karis 0, no threshold.  Level 1 is 1 x 1; its texel reads
columns and rows clampi(-2 .. 3, 2) = 0 0 0 1 1 1, so t[i][j] = 8 for i, j <= 2 and 0 elsewhere, and a quad Q(a, b) = 2 * n(a) * n(b)
with n = 2, 2, 1, 0, 0 for a = 0 .. 4:  Q(0,0) = 8, Q(2,0) = Q(0,2) = 4, Q(1,1) = 8, Q(2,2) = 2, every other quad 0.
inner = 8, edge = 8, corner = 8:  D_1 = (0.125 * (8 + 2) + 0.0625 * 8) + 0.03125 * 8 = (1.25 + 0.5) + 0.25 = 2, every step exact.
U_1 = D_1; up of a 1 x 1 level is that texel: B = 2 everywhere; strength 1: out = s + 1 * (2 - s) = 2 at all four pixels.

THE ENERGY FIGURE.  A 256 x 256 black frame with one pixel of (1000, 800, 600) at (128, 128), 4 levels (the coarsest is 16 x 16: the two
outermost rows and columns of every level stay 0, so no tap that carries light is clamped), threshold 0, karis 0, scatter 0.7,
strength 1.  Both filters spread a texel with a total weight of 1, so the sum of out3f is the sum of the input up to rounding.  The
numpy reference, its binary32 words summed in binary64: relative deviation ENERGY_DEVIATION below (measured, 4.5e-8); asserted on the
reference, the host build and the GPU: twice that.  A lost or doubled tap shows at 1 / 32 of the sum and above."""
import subprocess

import numpy as np
import pytest

import bloom_ref as R

F = np.float32
U32 = np.uint32
ENERGY_DEVIATION = 4.4834562610655364e-08       # measured on the numpy reference (profiles/bloom/README.md)
ENERGY_BOUND = 2 * ENERGY_DEVIATION
ENERGY_SETTING = dict(levels=4, karis=0, threshold=0.0, knee=0.0, scatter=0.7, strength=1.0, scale=1.0)


def test_program_checks_itself():
    out = subprocess.check_output([R.host_program()], text=True)
    assert "bloom_host: ok" in out


@pytest.mark.parametrize("run", [R.bloom, R.bloom_host], ids=["reference", "host"])
def test_the_case_by_hand(run):
    color = np.zeros((2, 2, 3), F)
    color[0, 0, 0] = 8.0
    out, B, D, U = run(color, levels=1, karis=0, scale=1.0, scatter=0.5, strength=1.0)
    assert len(D) == 1 and D[0].shape == (1, 1, 3) and D[0].reshape(-1).tolist() == [2.0, 0.0, 0.0] and R.differ(D[0], U[0]) == 0
    want = np.zeros((2, 2, 3), F)
    want[..., 0] = 2.0
    assert R.differ(out, want) == 0 and R.differ(B, want) == 0


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_build_equals_the_reference(size):
    W, H = size
    for name, kw in R.cases(W, H):
        ref = R.bloom(**kw)
        assert R.differ_all(R.bloom_host(**kw), ref) == 0, name
    for name, kw in R.cases(W, H)[:2]:
        assert R.differ_all(R.bloom_host(in_place=True, **kw), R.bloom(**kw)) == 0, name + " (in place)"


def test_the_cases_cover_what_they_name():
    """the sizes reach every route of the launch plan, and the inputs do what their names say, on the reference's own outputs"""
    assert [R.tail_first(W, H, 8) for W, H in R.SIZES] == [0, 0, 1, 1, 1, 1, 1, 1, 2]      # no tail; the tail from level 1; one level above it
    assert R.tail_first(130, 70, 8) == 1 and R.tail_first(300, 120, 8) == 2 and R.tail_first(300, 120, 8, variant=1) == 0
    assert len(R.level_sizes(3, 5, 8)) - 1 == 3 and R.level_sizes(3, 5, 8)[-1] == (1, 1)                # levels beyond the collapse are not made
    assert (R.launches(1920, 1080, 6, 0), R.launches(1920, 1080, 6, 1), R.launches(1920, 1080, 8, 0), R.launches(1920, 1080, 8, 1)) == (11, 12, 11, 16)
    W, H = 70, 66
    cs = dict(R.cases(W, H))
    assert {kw["levels"] for kw in cs.values()} >= set(R.LEVELS) and {kw.get("variant", 0) for kw in cs.values()} == {0, 1}
    # karis changes level 1, the threshold takes light away, a state replaces the exposure
    a, b = R.bloom(**cs["levels 2, karis"]), R.bloom(**dict(cs["levels 2, karis"], karis=0))
    assert R.differ(a[2][0], b[2][0]) > 0
    t = R.bloom(**cs["threshold alone"])
    assert t[1].astype(np.float64).sum() < 0.9 * R.bloom(**dict(cs["threshold alone"], threshold=0.0))[1].astype(np.float64).sum()
    kw = cs["knee above the threshold, a state"]
    assert R.differ(R.bloom(**kw)[1], R.bloom(**dict(kw, state_exposure=None))[1]) > 0
    kw = cs["a state without a threshold"]                       # ... and is never read without a prefilter
    assert R.differ(R.bloom(**kw)[1], R.bloom(**dict(kw, state_exposure=None))[1]) == 0
    # planted bad values: the input holds NaN, infinities, negative and huge channels; everything that leaves is finite and not negative
    kw = cs["planted bad"]
    c = kw["color"]
    assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and (c < 0).any() and (c[np.isfinite(c)] * F(kw["scale"]) > 2.0 ** 60).any()
    for name in ("planted bad", "planted bad, threshold, per level", "planted bad, a huge scale", "a state that is not finite", "a huge knee"):
        out, B, D, U = R.bloom(**cs[name])
        for plane in [out, B] + D + U:
            assert np.isfinite(plane).all() and (plane >= 0).all() and not np.signbit(plane).any(), name
    out, B, D, U = R.bloom(**cs["black"])
    assert not out.view(U32).any() and not B.view(U32).any()
    out, B, _, _ = R.bloom(**cs["a negative scale"])
    assert not out.view(U32).any() and not B.view(U32).any()
    # scatter 0: the bloom is level 1 alone, upsampled; scatter 1: U_k is up(U_(k+1)) -- the coarsest level's light alone
    kw = cs["scatter 0 strength 1"]
    out, B, D, U = R.bloom(**kw)
    assert R.differ(B, R.up(D[0], W, H)) == 0 and R.differ(U[0], D[0]) == 0


# ---- the properties: run(color, **settings) -> (out, bloom, ...) ------------------------------------------------------------------
def strength_zero_gives_the_sanitised_colour(run):
    for W, H in ((33, 31), (130, 70)):
        c = R.planted_bad(R.frame(W, H))
        for kw in (dict(levels=8, karis=1, scale=0.25), dict(levels=2, karis=0, scale=0.25, threshold=1.0, knee=0.5, variant=1)):
            out = run(c, strength=0.0, **kw)[0]
            assert R.differ(out, R.sanitise(c, 0.25)) == 0, (W, H, kw)


def constant_frames_stay_constant(run, sizes=R.SIZES):
    """0.5 and 3.0: every partial sum is exact, so any edge clamp or parity slip that takes a texel twice or not at all shows"""
    for W, H in sizes:
        for v in (0.5, 3.0):
            for levels, variant in ((8, 0), (2, 1)):
                c = np.full((H, W, 3), v, F)
                got = run(c, levels=levels, karis=0, scale=1.0, scatter=0.7, strength=0.5, variant=variant)
                assert R.differ(got[0], c) == 0 and R.differ(got[1], c) == 0, (W, H, v, levels)
                for level in list(got[2]) + list(got[3]) if len(got) > 2 else []:
                    assert (level == F(v)).all(), (W, H, v, levels)


def non_finite_input_gives_finite_output(run):
    c = R.planted_bad(R.frame(70, 66))
    c[::3, ::5, 1] = np.nan
    c[1::7, 2::3] = np.inf
    for kw in (dict(levels=8, karis=1, scale=0.25, strength=0.5), dict(levels=8, karis=0, scale=1.0, threshold=0.5, knee=0.25, exposure=2.0, strength=1.0)):
        out, B = run(c, **kw)[:2]
        assert np.isfinite(out).all() and np.isfinite(B).all() and (out >= 0).all() and (B >= 0).all() and B.any()


def spike_frame():
    c = np.zeros((256, 256, 3), F)
    c[128, 128] = (1000.0, 800.0, 600.0)
    return c


def energy_deviation(run):
    """(sum of out - sum of the input) / sum of the input, binary64 sums of binary32 words"""
    c = spike_frame()
    out = run(c, **ENERGY_SETTING)[0]
    s = c.astype(np.float64).sum()
    return (out.astype(np.float64).sum() - s) / s


def energy_is_conserved(run):
    d = energy_deviation(run)
    print("energy: relative deviation %.17g, bound %.17g" % (d, ENERGY_BOUND))
    assert abs(d) <= ENERGY_BOUND


PROPERTIES = [strength_zero_gives_the_sanitised_colour, constant_frames_stay_constant, non_finite_input_gives_finite_output, energy_is_conserved]


@pytest.mark.parametrize("prop", PROPERTIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("run", [R.bloom, R.bloom_host], ids=["reference", "host"])
def test_properties(run, prop):
    prop(run)


def test_the_energy_frame_clamps_no_tap_that_carries_light():
    """the two outermost rows and columns of every level, after either sweep, are 0: what 'no level's footprint reaches an edge' means;
    and the recorded figure is the reference's"""
    out, B, D, U = R.bloom(spike_frame(), **ENERGY_SETTING)
    for level in D + U:
        assert level.shape[0] >= 16 and not level[:2].any() and not level[-2:].any() and not level[:, :2].any() and not level[:, -2:].any()
    assert energy_deviation(R.bloom) == pytest.approx(ENERGY_DEVIATION, rel=1e-6)
