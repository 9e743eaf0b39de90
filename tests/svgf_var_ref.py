"""Reference of art_denoise_svgf_var_device written from the header comment of include/art_hip.h: tests/svgf_ref.py's denoise() with the
preparation of v_0 the header states for the variance plane, everything after it the same text.  Also the g++ build of the product's
text behind tests/temporal_host/libtemporal_host.so, and the variance plane that belongs to a pair of moments.

Why denoise_var repeats the body of svgf_ref.denoise: that function derives v_0 from the moments inside itself and offers no seam to hand
it another v_0, and tests/svgf_ref.py is an existing yardstick that stays byte for byte.  The two bodies are held together by
tests/test_svgf_var_reference_host.py::test_equals_the_moments_entrance_where_the_header_says_so, which fails as soon as they drift.  For
the same reason the g++ functions live in tests/temporal_host and not in tests/svgf_host."""
import ctypes as C
import itertools

import numpy as np

import svgf_ref as S
import temporal_ref as T
from denoise_ref import F, SPLINE, _finite3, _lum, _shift, exp_small
from svgf_ref import KK


def denoise_var(color, variance, albedo=None, normal=None, depth=None, iterations=5, scale=1.0, sigma_color=4.0, sigma_depth=1.0,
            normal_log2=7, demodulate=True):
    """color, albedo, normal [H, W, 3], variance, depth [H, W] float32 -> (out [H, W, 3], variance [H, W]) float32"""
    with np.errstate(all="ignore"):
        color = np.asarray(color, F)
        H, W = color.shape[:2]
        variance = np.asarray(variance, F).reshape(H, W)
        scale, sigma_color, sigma_depth = F(scale), F(sigma_color), F(sigma_depth)
        c = scale * color
        demod = bool(demodulate) and albedo is not None
        if demod:
            albedo = np.asarray(albedo, F)
            a = np.where(albedo >= F(1e-3), albedo, F(1e-3)).astype(F)
            c = c / a
        # v_0 from the variance plane, binary64 with one rounding to binary32
        v64 = variance.astype(np.float64) * (np.float64(scale) * np.float64(scale))
        if demod:
            la = _lum(a).astype(np.float64)
            v64 = v64 / (la * la)
        v = v64.astype(F)
        no_stop = ~np.isfinite(v)
        v = np.where(no_stop, F(0), v).astype(F)
        bad_guides = np.zeros((H, W), bool)
        if normal is not None:
            normal = np.asarray(normal, F)
            bad_guides |= ~_finite3(normal)
        use_depth = depth is not None and sigma_depth > 0
        if depth is not None:
            z = np.asarray(depth, F)
            bad_guides |= ~np.isfinite(z)
            xi, yi = np.arange(W), np.arange(H)
            gx = F(0.5) * (z[:, np.minimum(xi + 1, W - 1)] - z[:, np.maximum(xi - 1, 0)])
            gy = F(0.5) * (z[np.minimum(yi + 1, H - 1), :] - z[np.maximum(yi - 1, 0), :])
            zfloor = F(1e-3) * z + F(1e-6)
        for i in range(iterations):
            s = 1 << i
            centre_bad = ~_finite3(c)
            # the variance prefilter
            vs, ks = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy, dx in itertools.product(range(-1, 2), range(-1, 2)):
                cq, inside = _shift(c, dx, dy)
                vq, _ = _shift(v, dx, dy)
                bq, _ = _shift(bad_guides, dx, dy)
                take = inside & ~bq & _finite3(cq)
                k = KK[abs(dx)] * KK[abs(dy)]
                vs = np.where(take, vs + k * vq, vs)
                ks = np.where(take, ks + k, ks)
            vg = np.where(ks > 0, vs / np.where(ks > 0, ks, F(1)), F(0)).astype(F)
            sc = (sigma_color * np.sqrt(vg) + F(1e-6)).astype(F)
            acc = np.zeros((H, W, 3), F)
            av = np.zeros((H, W), F)
            wsum = np.zeros((H, W), F)
            lp = _lum(c)
            for dy, dx in itertools.product(range(-2, 3), range(-2, 3)):
                cq, inside = _shift(c, s * dx, s * dy)
                vq, _ = _shift(v, s * dx, s * dy)
                bq, _ = _shift(bad_guides, s * dx, s * dy)
                take = inside & ~bq & _finite3(cq)
                h = SPLINE[abs(dx)] * SPLINE[abs(dy)]
                if dx == 0 and dy == 0:
                    w = np.full((H, W), h, F)
                else:
                    wn = np.ones((H, W), F)
                    if normal is not None:
                        nq, _ = _shift(normal, s * dx, s * dy)
                        d = (normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]) + normal[..., 2] * nq[..., 2]
                        wn = np.where(d >= F(0), d, F(0)).astype(F)
                        for _ in range(normal_log2):
                            wn = wn * wn
                    xz = np.zeros((H, W), F)
                    if use_depth:
                        zq, _ = _shift(z, s * dx, s * dy)
                        xz = np.abs(z - zq) / (sigma_depth * (np.abs(gx * F(s * dx)) + np.abs(gy * F(s * dy))) + zfloor)
                    xc = np.zeros((H, W), F)
                    if sigma_color > 0:
                        xc = np.where(centre_bad | no_stop, F(0), np.abs(lp - _lum(cq)) / sc).astype(F)
                    t = -(xz.astype(np.float64) + xc.astype(np.float64))
                    e = np.full((H, W), np.nan, F)
                    e[t < -200.0] = 0.0
                    m = (t >= -200.0) & (t <= 0.0)
                    e[m] = exp_small(t[m]).astype(F)
                    w = (h * wn) * e
                    take &= ~np.isnan(w)
                assert w.dtype == F and cq.dtype == F and vq.dtype == F
                acc = np.where(take[..., None], acc + w[..., None] * cq, acc)
                av = np.where(take, av + (w * w) * vq, av)
                wsum = np.where(take, wsum + w, wsum)
            ok = wsum > 0
            one = np.where(ok, wsum, F(1))
            c = np.where(ok[..., None], acc / one[..., None], c).astype(F)
            v = np.where(ok, av / (one * one), v).astype(F)
        return (c * a if demod else c).astype(F), v


def denoise_var_host(color, variance, albedo=None, normal=None, depth=None, iterations=5, scale=1.0, sigma_color=4.0, sigma_depth=1.0,
                     normal_log2=7, demodulate=True):
    """the same call through csrc/art_denoise.h compiled by g++"""
    arrs = [None if x is None else np.ascontiguousarray(x, F) for x in (color, variance, albedo, normal, depth)]
    H, W = arrs[0].shape[:2]
    out, var = np.zeros((H, W, 3), F), np.zeros((H, W), F)
    p = S.Params(W, H, iterations, 1 if demodulate else 0, normal_log2, 0, scale, sigma_color, sigma_depth)
    rc = T.host_lib().th_denoise_svgf_var(C.addressof(p), *[None if x is None else x.ctypes.data for x in arrs], out.ctypes.data, var.ctypes.data)
    if rc:
        raise RuntimeError("th_denoise_svgf_var refused its arguments")
    return out, var


def variance_of(moments, n_colours):
    """(float)(D0 * (n / (n - 1))) of art_denoise_svgf_device's own formula: the plane that stands for {S1, S2} and n"""
    with np.errstate(all="ignore"):
        n = np.float64(n_colours)
        s1, s2 = moments[..., 0].astype(np.float64), moments[..., 1].astype(np.float64)
        D = s2 - (s1 * s1) / n
        return (np.where(D < 0.0, 0.0, D) * (n / (n - 1.0))).astype(F)


def variance_plane(color, W, H, seed=0):
    """a variance plane for `color`: variance_of tests/svgf_ref.py's moments, with a few entries that are not finite or negative"""
    v = variance_of(S.moments_for(color, 4, W, H, seed), 4)
    rng = np.random.default_rng(5 * W + H + seed)
    v[rng.random((H, W)) < 0.05] = np.inf
    if W * H > 6:
        v.reshape(-1)[3] = np.nan; v.reshape(-1)[5] = -1.0
    return v
