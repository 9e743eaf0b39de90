"""Reference of art_denoise_svgf_device written from the header comment of include/art_hip.h alone: plain numpy over the pixels, binary32
arrays except where the header names binary64, Python loops over the iterations and the taps.  exp_small, the shifted views and the
shared input planes are those of tests/denoise_ref.py.  Also the loader of tests/svgf_host/libsvgf_host.so -- the product's per-pixel text
(csrc/art_denoise.h, csrc/art_shade.h accumulate_pixel_moments) compiled by g++."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

import denoise_ref as R
from denoise_ref import F, SPLINE, _finite3, _lum, _shift, differ, exp_small      # noqa: F401 (differ: for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
KK = (F(0.5), F(0.25))


def denoise(color, moments, n_colours, albedo=None, normal=None, depth=None, iterations=5, scale=1.0, sigma_color=4.0, sigma_depth=1.0,
            normal_log2=7, demodulate=True):
    """color, albedo, normal [H, W, 3], moments [H, W, 2], depth [H, W] float32 -> (out [H, W, 3], variance [H, W]) float32"""
    with np.errstate(all="ignore"):
        color = np.asarray(color, F)
        H, W = color.shape[:2]
        moments = np.asarray(moments, F).reshape(H, W, 2)
        scale, sigma_color, sigma_depth = F(scale), F(sigma_color), F(sigma_depth)
        c = scale * color
        demod = bool(demodulate) and albedo is not None
        if demod:
            albedo = np.asarray(albedo, F)
            a = np.where(albedo >= F(1e-3), albedo, F(1e-3)).astype(F)
            c = c / a
        # v_0, binary64 with one rounding to binary32
        n = np.float64(n_colours)
        s1, s2 = moments[..., 0].astype(np.float64), moments[..., 1].astype(np.float64)
        D = s2 - (s1 * s1) / n
        D0 = np.where(D < 0.0, 0.0, D)
        v64 = (D0 * (n / (n - 1.0))) * (np.float64(scale) * np.float64(scale))
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


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
class Params(C.Structure):          # include/art_hip.h ArtSvgfParams (its own mirror: the host library needs no package)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("demodulate", C.c_int32),
                ("normal_log2", C.c_int32), ("n_colours", C.c_int32), ("scale", C.c_float), ("sigma_color", C.c_float), ("sigma_depth", C.c_float)]


_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "svgf_host"), "libsvgf_host.so"])
        L = C.CDLL(os.path.join(HERE, "svgf_host", "libsvgf_host.so"))
        L.sh_denoise_svgf.argtypes = [C.POINTER(Params)] + [C.c_void_p] * 7
        L.sh_denoise_svgf.restype = C.c_int
        L.sh_accumulate.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sh_accumulate.restype = C.c_int
        _host = L
    return _host


def denoise_host(color, moments, n_colours, albedo=None, normal=None, depth=None, iterations=5, scale=1.0, sigma_color=4.0, sigma_depth=1.0,
                 normal_log2=7, demodulate=True):
    """the same call through csrc/art_denoise.h compiled by g++"""
    arrs = [None if x is None else np.ascontiguousarray(x, F) for x in (color, moments, albedo, normal, depth)]
    H, W = arrs[0].shape[:2]
    out, var = np.zeros((H, W, 3), F), np.zeros((H, W), F)
    p = Params(W, H, iterations, 1 if demodulate else 0, normal_log2, n_colours, scale, sigma_color, sigma_depth)
    rc = host_lib().sh_denoise_svgf(C.byref(p), *[None if x is None else x.ctypes.data for x in arrs], out.ctypes.data, var.ctypes.data)
    if rc:
        raise RuntimeError("sh_denoise_svgf refused its arguments")
    return out, var


def accumulate_host(rad, aa_on, background, accum, moments, pixmap=None):
    """csrc/art_shade.h through g++: one batch of rad [S, npix, 3] added into accum [frame pixels, 3] and moments [frame pixels, 2], by
    accumulate_pixel_moments; and into a copy of accum by accumulate_pixel.  Returns (accum, moments, accum of accumulate_pixel)."""
    rad = np.ascontiguousarray(rad, F)
    S, npix = rad.shape[:2]
    planes = np.ascontiguousarray(rad.transpose(2, 0, 1))             # rad_r, rad_g, rad_b: [S, npix] each
    bg = np.ascontiguousarray(background, F)
    a, m = np.array(accum, F, copy=True), np.array(moments, F, copy=True)
    plain = np.array(accum, F, copy=True)
    pm = None if pixmap is None else np.ascontiguousarray(pixmap, np.uint32)
    rc = host_lib().sh_accumulate(npix, S, int(aa_on), planes.ctypes.data, bg.ctypes.data, None if pm is None else pm.ctypes.data,
                                  a.ctypes.data, m.ctypes.data, plain.ctypes.data)
    assert rc == 0
    return a, m, plain


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
SIZES = R.SIZES if (1, 1) in R.SIZES else R.SIZES + [(1, 1)]          # (W, H): denoise_ref.SIZES plus 1 x 1
GPU_SIZES = SIZES + [(64, 4), (65, 4), (63, 3), (300, 5)]             # a full workgroup row, one pixel over, one under, more than one workgroup


def moments_for(color, n_colours, W, H, seed=0):
    """moments that belong to `color` read as the sum of n colours: S1 = lum(color), S2 from a relative spread log-uniform over
    1e-3 .. 10, so that the standard deviation lies on both sides of the luminance differences between neighbours; some pixels with
    zero spread (S2 = S1^2 / n: D is a rounding residue of either sign, the clamp's case)"""
    rng = np.random.default_rng(77 * W + H + seed)
    s1 = _lum(np.asarray(color, F)).astype(np.float64)
    rel = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), (H, W)))
    rel[rng.random((H, W)) < 0.15] = 0.0
    s2 = s1 * s1 / n_colours * (1.0 + rel * rel)
    return np.stack([s1, s2], axis=-1).astype(F)


def combos():
    """(iterations, guides subset, demodulate, sigma_color, n_colours, normal_log2): the full cross of the 8 guide subsets x demodulate
    on / off x sigma_color 0, 1, 4 (48), with iterations 1, 2, 3, n_colours 2, 64 and normal_log2 7, 0 dealt over them in rotation; plus
    iterations 1, 5 and 8 with every guide on (the GPU test runs 5 and 8 at 37 x 23 only)"""
    subsets = [tuple(g for g, on in zip(("albedo", "normal", "depth"), bits) if on) for bits in itertools.product((0, 1), repeat=3)]
    out = []
    for k, (sub, dm, sc) in enumerate(itertools.product(subsets, (0, 1), (0.0, 1.0, 4.0))):
        out.append(((1, 2, 3)[k % 3], sub, dm, sc, (2, 64)[k % 2], (7, 0)[(k // 2) % 2]))
    full = ("albedo", "normal", "depth")
    out += [(1, full, 1, 4.0, 2, 7), (5, full, 1, 4.0, 64, 7), (8, full, 1, 2.0, 8, 7)]
    return out


def combo_id(c):
    return "i%d-%s-d%d-sc%g-n%d-l%d" % (c[0], "".join(g[0] for g in c[1]) or "none", c[2], c[3], c[4], c[5])


def combo_args(pl, c, W, H):
    """denoise_ref.planes() and one of combos() -> (color, moments, n_colours, dict of the guides given, dict of the parameters)"""
    color, albedo, normal, depth = pl
    it, sub, dm, sc, nc, nl = c
    kw = dict(iterations=it, demodulate=bool(dm), sigma_color=sc, normal_log2=nl, scale=0.25, sigma_depth=1.0)
    g = dict(albedo=albedo if "albedo" in sub else None, normal=normal if "normal" in sub else None, depth=depth if "depth" in sub else None)
    return color, moments_for(color, nc, W, H), nc, g, kw
