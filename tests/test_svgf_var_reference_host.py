"""art_denoise_svgf_var_device without a GPU: csrc/art_denoise.h's svgf_var_pack_pixel + svgf_atrous_pixel compiled by g++ against the
numpy reference (tests/svgf_var_ref.py), bit for bit; and against the moments entrance where the header says the two agree."""
import numpy as np
import pytest

import denoise_ref as R
import svgf_ref as S
import svgf_var_ref as V

F = np.float32


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_build_equals_the_numpy_reference(size):
    W, H = size
    pl = R.planes(W, H)
    var = V.variance_plane(pl[0], W, H)
    for c in S.combos():
        color, _, _, g, kw = S.combo_args(pl, c, W, H)
        got, want = V.denoise_var_host(color, var, **g, **kw), V.denoise_var(color, var, **g, **kw)
        assert S.differ(got[0], want[0]) == 0 and S.differ(got[1], want[1]) == 0, S.combo_id(c)


@pytest.mark.parametrize("fn", [V.denoise_var, V.denoise_var_host], ids=["numpy", "host_build"])
def test_a_variance_that_is_not_finite_is_no_colour_stop(fn):
    """+inf (temporal's "fewer than two colours"), NaN: v_0 = 0 and the centre has no colour stop -- the result at that centre is the
    result with sigma_color = 0 there; a negative variance is taken as it is (the header sets no clamp)"""
    W, H = 9, 7
    color = R.planes(W, H)[0]
    var = np.full((H, W), np.inf, F)
    a = fn(color, var, iterations=1, sigma_color=2.0)
    b = fn(color, np.zeros((H, W), F), iterations=1, sigma_color=0.0)
    assert S.differ(a[0], b[0]) == 0 and not a[1].any()


@pytest.mark.parametrize("size", [(7, 5), (37, 23)], ids=lambda s: "%dx%d" % s)
def test_equals_the_moments_entrance_where_the_header_says_so(size):
    """scale a power of two and no demodulation: (float)(D0 * n / (n - 1)) as the plane gives art_denoise_svgf_device's bits"""
    W, H = size
    color, albedo, normal, depth = R.planes(W, H)
    for nc in (2, 64):
        mom = S.moments_for(color, nc, W, H)
        var = V.variance_of(mom, nc)
        for fn_m, fn_v in ((S.denoise, V.denoise_var), (S.denoise_host, V.denoise_var_host)):
            kw = dict(normal=normal, depth=depth, iterations=2, scale=0.25, sigma_color=2.0)
            a, b = fn_m(color, mom, nc, **kw), fn_v(color, var, **kw)
            assert S.differ(a[0], b[0]) == 0 and S.differ(a[1], b[1]) == 0


def test_params_are_refused_by_the_host_build():
    color, var = np.ones((2, 2, 3), F), np.ones((2, 2), F)
    for kw in (dict(iterations=0), dict(iterations=9), dict(normal_log2=11), dict(scale=np.inf), dict(sigma_color=np.nan)):
        with pytest.raises(RuntimeError):
            V.denoise_var_host(color, var, **kw)
