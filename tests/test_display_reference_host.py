"""art_auto_exposure_device and art_display_device without a GPU: the product's text (csrc/art_display.h) compiled by g++ as a stand-alone
program against the numpy reference written from the header (tests/display_ref.py), bit for bit, on the frames and cases the GPU test
shares: every screen word, every ldr word, every histogram bin and the four state words; the program's own checks; the reference curve
against the oracle's resolve; and what follows from the arithmetic without trimming."""
import subprocess

import numpy as np
import pytest

import display_ref as D

F = np.float32
SIZE_IDS = lambda s: "%dx%d" % s


def test_program_checks_itself():
    out = subprocess.check_output([D.host_program()], text=True)
    assert "display_host: ok" in out


@pytest.mark.parametrize("size", D.SIZES, ids=SIZE_IDS)
def test_exposure_host_build_equals_the_reference(size):
    W, H = size
    for name, frames, kw in D.exposure_cases(W, H):
        ref, host = D.new_state(), D.new_state()
        for k, frame in enumerate(frames):
            ref, host = D.auto_exposure(frame, ref, **kw), D.auto_exposure_host(frame, host, **kw)
            assert D.differ(ref[4:], host[4:]) == 0, "%s, frame %d: histogram" % (name, k)
            assert D.differ(ref[:4], host[:4]) == 0, "%s, frame %d: state words %s != %s" % (name, k, ref[:4], host[:4])
            assert int(ref[4:].sum()) == W * H and ref[4 + 255] == 0


@pytest.mark.parametrize("size", D.SIZES, ids=SIZE_IDS)
def test_display_host_build_equals_the_reference(size):
    W, H = size
    for name, kw in D.display_cases(W, H):
        screen, ldr = D.display(**kw)
        hs, hl = D.display_host(**kw)
        assert D.differ(screen, hs) == 0, name + ": screen"
        assert (ldr is None) == (hl is None) and (ldr is None or D.differ(ldr, hl) == 0), name + ": ldr"
        assert int((screen >> 24).max()) == 0 and (ldr is None or (np.isfinite(ldr).all() and ldr.min() >= 0 and ldr.max() <= F(1.0000001)))


def product(frame, state, **kw):
    """the state after the call by the g++ build of csrc/art_display.h -- the product's text -- which the numpy reference must give too"""
    host = D.auto_exposure_host(frame, state, **kw)
    assert D.differ(host, D.auto_exposure(frame, state, **kw)) == 0
    return host


def test_one_output_alone():
    W, H = 37, 23
    for name, kw in D.display_cases(W, H)[20:28]:
        screen, ldr = D.display(**kw)
        hs, hl = D.display_host(want_ldr=False, **kw)
        assert hl is None and D.differ(screen, hs) == 0, name
        if ldr is not None:
            hs, hl = D.display_host(want_screen=False, **kw)
            assert hs is None and D.differ(ldr, hl) == 0, name


def test_the_cases_cover_what_they_name():
    """the inputs do what their names say, and the properties the cases are named for hold of the product: every state below is the g++
    build's (product()), which the numpy reference equals word for word"""
    W, H = 67, 131
    cs = {name: (frames, kw) for name, frames, kw in D.exposure_cases(W, H)}
    c = D.special_frame(W, H)
    l = D.lum(c.reshape(-1, 3))
    with np.errstate(all="ignore"):
        assert np.isnan(l).any() and np.isinf(l).any() and (l < 0).any() and (l == 0).any() and ((l > 0) & (l < F(1.2e-38))).any()
        assert (l == F(2.0 ** -4)).any() and (l == F(2.0 ** -12)).any() and (l == F(2.0 ** 4)).any() and (l > F(16)).any() and ((l > 0) & (l < F(2.0 ** -12))).any()
    h = product(c, D.new_state())[4:]
    assert h[0] >= 6 and h[1] > 0 and h[254] > 0 and h[255] == 0
    # the luminance 2^-4 and its lower neighbour fall either side of the edge between bins 127 and 128 (words 4 + 127, 4 + 128)
    g = D.green_of_luminance(2.0 ** -4)
    at = lambda g: int(np.nonzero(product(np.array([[[0, g, 0]]], F), D.new_state())[4:])[0][0])
    assert at(np.nextafter(g, F(0))) == 127 and at(np.nextafter(g, F(1))) == 128 and at(g) in (127, 128)
    frames, kw = cs["one_bin"]
    assert (product(frames[0], D.new_state())[5:] != 0).sum() == 1
    frames, kw = cs["black_fresh_then_valid"]
    s = product(frames[0], D.new_state(), **kw)
    assert D.exposure_of(s) == 1 and s[2] == 0 and s[3] == 0 and s[4] == W * H
    s1 = product(frames[1], s, **kw)
    assert s1[3] == 1 and D.differ(s1[:4], product(frames[1], D.new_state(), **kw)[:4]) == 0      # the black frame left no trace: a jump, not a blend
    frames, kw = cs["black_after_valid"]
    s = product(frames[0], D.new_state(), **kw)
    for f in frames[1:3]:
        t = product(f, s, **kw)
        assert D.differ(t[:2], s[:2]) == 0 and t[2] == 0 and t[3] == 1
    frames, kw = cs["adapt_quarter"]
    s = D.new_state()
    es, ts = [], []
    for f in frames:
        s = product(f, s, **kw)
        es.append(float(D.exposure_of(s))); ts.append(float(D.exposure_of(product(f, D.new_state(), **kw))))
    assert es[0] == ts[0] and abs(es[1] - (es[0] + 0.25 * (ts[1] - es[0]))) < 1e-6 * es[0] and abs(es[2] - (es[1] + 0.25 * (ts[2] - es[1]))) < 1e-6 * es[1]
    assert es[1] != ts[1]                                            # the state after frame 2 depends on frame 1's
    frames, kw = cs["clamped_to_the_bounds"]
    s = product(frames[0], D.new_state(), **kw)
    assert D.exposure_of(s) in (F(0.5), F(2.0)) and D.exposure_of(product(frames[1], D.new_state(), **kw)) == F(2.0)
    a = D.exposure_of(product(cs["range_ends_inside_a_bin"][0][0], D.new_state(), **cs["range_ends_inside_a_bin"][1]))
    b = D.exposure_of(product(cs["range_ends_inside_a_bin"][0][0], D.new_state(), low_fraction=0.123, high_fraction=0.7771))
    assert a != b                                                    # a rank range that ends inside a bin: the end's position counts


def test_without_trimming_the_exposure_is_the_mean_of_the_bin_centres():
    """derived, not measured.  With no trimming and adapt = 1 every counted pixel weighs 1, so -log2(exposure / key) is the mean of the
    counted pixels' bin centres, to the roundings of m (binary32, 2^-24 relative on |m| < 16) and of key * apow (two more): 1e-5 holds
    them with room.  A bin's centre is within half a bin width of every log2 luminance in the bin, so that mean differs from the exact
    mean log2 luminance by at most half a bin width, (max_log2 - min_log2) / 508, on a frame inside the range."""
    for W, H in D.SIZES[1:]:
        c = D.hdr_frame(W, H, 11, 1e-3, 15.0)                       # every luminance inside 2^-12 .. 2^4: no pixel is clamped into an end bin
        l2 = np.log2(D.lum(c.reshape(-1, 3)).astype(np.float64))
        assert l2.min() > -12.0 and l2.max() < 4.0
        kw = dict(low_fraction=0.0, high_fraction=1.0, adapt=1.0)
        s = product(c, D.new_state(), **kw)                        # the product's state words: the bound below is asserted of them
        hist = s[4:].astype(np.float64)
        assert hist[0] == 0 and s[2] == W * H
        centres = -12.0 + ((np.arange(256) - 1 + 0.5) / 254.0) * 16.0
        mean_centres = (hist[1:255] * centres[1:255]).sum() / hist[1:255].sum()
        got = -np.log2(float(D.exposure_of(s)) / float(F(0.18)))
        assert abs(got - mean_centres) < 1e-5
        assert abs(float(s[1:2].view(F)[0]) - mean_centres) < 1e-6
        exact = l2.mean()
        print("%dx%d: -log2(exposure / key) %.6f, mean of centres %.6f, exact mean log2 luminance %.6f, bound %.6f" % (W, H, got, mean_centres, exact, 16.0 / 508))
        assert abs(got - exact) <= 16.0 / 508


def test_reference_curve_is_the_oracles_resolve():
    """ART_CURVE_REFERENCE against the CPU oracle's resolve (oracle/art_oracle.c, what art_download's screen is held to) on a frame of
    finite, non-negative sums, in both layouts: the numpy reference and the g++ build give its words"""
    import orc
    W, H, spp = 37, 23, 4
    c = D.hdr_frame(W, H, 3, 1e-3, 8.0)
    c[D.spots(H, W, 0)] = 0
    want = orc.resolve(c, spp)
    for layout in D.layouts(W, H):
        w = want if layout == D.LAYOUT_ROW_MAJOR else np.ascontiguousarray(want.T)
        kw = dict(color=c, scale=1.0 / spp, curve=D.CURVE_REFERENCE, layout=layout)
        assert D.differ(D.display(**kw)[0], w) == 0 and D.differ(D.display_host(**kw)[0], w) == 0
