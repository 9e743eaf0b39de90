"""art_svgf_spatial_variance_device without a GPU: the product's per-pixel text (csrc/art_svgf_spatial.h) compiled by g++ against the
numpy reference written from the header (tests/svgf_spatial_ref.py), bit for bit, on the synthetic cases the GPU test shares; the
stand-alone program's own checks; and the fixed point -- where the stops shut every neighbour out the call gives art_temporal_device's
own variance (tests/temporal_ref.py) word for word."""
import subprocess

import numpy as np
import pytest

import svgf_spatial_ref as SP
import temporal_ref as T

F = np.float32


def test_program_checks_itself():
    out = subprocess.check_output([SP.host_program()], text=True)
    assert "svgf_spatial_host: ok" in out


@pytest.mark.parametrize("radius", SP.RADII)
@pytest.mark.parametrize("size", SP.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_build_equals_the_reference(size, radius):
    W, H = size
    for name, kw in SP.cases(W, H):
        ref = SP.spatial(radius=radius, **kw)
        assert SP.differ(SP.spatial_host(radius=radius, **kw), ref) == 0, name
        assert SP.differ(SP.spatial_host(radius=radius, in_place=True, **kw), ref) == 0, name + " (in place)"


def test_the_cases_cover_what_they_name():
    """the inputs do what their names say, on the reference's own outputs"""
    W, H = 37, 29
    cs = dict(SP.cases(W, H))
    inf = lambda v: np.isinf(v) & (v > 0)
    kw = cs["all_short"]
    assert inf(kw["variance"]).all()                                  # one colour: art_temporal_device says +inf everywhere
    out = SP.spatial(radius=3, **kw)
    assert np.isfinite(out).all() and (out > 0).all()                 # and the window finds a variance at every pixel
    kw = cs["all_long"]
    assert SP.differ(SP.spatial(radius=3, **kw), kw["variance"]) == 0
    kw = cs["checkerboard"]
    out = SP.spatial(radius=1, **kw)
    long_ = kw["hist"][0, ..., 3] >= 4
    assert 0 < long_.sum() < W * H and SP.differ(out[long_], kw["variance"][long_]) == 0 and np.isfinite(out[~long_]).all()
    kw = cs["single_short_pixel"]
    out = SP.spatial(radius=3, **kw)
    assert (out.view(np.uint32) != kw["variance"].view(np.uint32)).sum() == 1
    kw = cs["variance_in_not_finite_at_long_pixels"]
    out = SP.spatial(radius=2, **kw)
    assert (~np.isfinite(kw["variance"])).sum() == 3 and np.isfinite(out).all()
    kw = cs["bad_words_short"]
    out = SP.spatial(radius=3, **kw)
    nan = np.isnan(out)
    assert (out.view(np.uint32)[nan] == 0x7fc00000).all()
    a, b = SP.spatial(radius=3, **cs["depth_step_and_normal_flip"]), SP.spatial(radius=3, **dict(cs["depth_step_and_normal_flip"], sigma_depth=0.0))
    assert SP.differ(a, b) > 0                                        # the depth stop changes the estimate across the step


def test_fixed_point_is_temporals_own_variance():
    """histories made without a normal plane hold zero normals: every neighbour weighs 0, only the centre counts, and the estimate of
    every pixel is step 6 of art_temporal_device -- the plane the reference of that call returns, word for word (no NaN in it)"""
    W, H = 37, 29
    for nc, frames in ((1, 1), (2, 1), (1, 3), (3, 2)):
        h, prev, res = None, None, None
        for k in range(frames):
            c = T.cam((0.05 * k, 0.01 * k, 0.0))
            fr = dict(T.frame(c, W, H, seed=k, n_colours=nc), normal=None)
            res = T.temporal(n_colours=nc, cam_cur=c, cam_prev=prev, hist=h, scale=1.0 / nc, max_history=16, **fr)
            h, prev = res[0], c
        assert not np.isnan(res[2]).any() and (np.isinf(res[2]).all() if nc * frames == 1 else np.isfinite(res[2]).any())
        for radius in SP.RADII:
            for sd in (1.0, 0.0):
                kw = dict(hist=res[0], variance=res[2], radius=radius, min_history=np.inf, sigma_depth=sd)
                assert SP.differ(SP.spatial(**kw), res[2]) == 0 and SP.differ(SP.spatial_host(**kw), res[2]) == 0, (nc, frames, radius, sd)
