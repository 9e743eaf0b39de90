"""Reference of art_denoise_device written from the header comment of include/art_hip.h alone: plain numpy, binary32 arrays over the
pixels, Python loops over the iterations and the 25 taps, and its own transcription of exp_small (binary64 Horner, the coefficients as
hex literals).  Also the loader of tests/denoise_host/libdenoise_host.so -- the product's per-pixel text (csrc/art_denoise.h) compiled by
g++ -- and the inputs the denoiser's tests share."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
fh = float.fromhex

LOG2E, LN2_HI, LN2_LO = fh("0x1.71547652b82fep+0"), fh("0x1.62e42fee00000p-1"), fh("0x1.a39ef35793c76p-33")
EXP_C = [fh(c) for c in ("0x1.6124613a86d09p-33", "0x1.1eed8eff8d898p-29", "0x1.ae64567f544e4p-26", "0x1.27e4fb7789f5cp-22",
                         "0x1.71de3a556c734p-19", "0x1.a01a01a01a01ap-16", "0x1.a01a01a01a01ap-13", "0x1.6c16c16c16c17p-10",
                         "0x1.1111111111111p-7", "0x1.5555555555555p-5", "0x1.5555555555555p-3")] + [0.5, 1.0, 1.0]
SPLINE = (F(0.375), F(0.25), F(0.0625))


def exp_small(t):
    """binary64 array, -200 <= t <= 0 -> exp(t) as the header spells it"""
    t = np.asarray(t, np.float64)
    v = t * LOG2E
    k = np.trunc(v + np.where(v >= 0.0, 0.5, -0.5))
    r = (t - k * LN2_HI) - k * LN2_LO
    q = np.full_like(t, EXP_C[0])
    for c in EXP_C[1:]:
        q = q * r + c
    return q * np.ldexp(1.0, k.astype(np.int64))


def _finite3(c):
    return np.isfinite(c).all(axis=-1)


def _lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _shift(a, ox, oy, fill=0):
    """b[y, x] = a[y + oy, x + ox] where that lies inside the image (else fill), and the mask of those pixels"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    ys, ye = max(0, -oy), min(H, H - oy)
    xs, xe = max(0, -ox), min(W, W - ox)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + oy:ye + oy, xs + ox:xe + ox]
        inside[ys:ye, xs:xe] = True
    return b, inside


def denoise(color, albedo=None, normal=None, depth=None, iterations=5, scale=1.0, sigma_color=4.0, sigma_depth=1.0, normal_log2=7,
            demodulate=True):
    """color, albedo, normal [H, W, 3], depth [H, W] float32 -> out [H, W, 3] float32"""
    with np.errstate(all="ignore"):
        color = np.asarray(color, F)
        H, W = color.shape[:2]
        scale, sigma_color, sigma_depth = F(scale), F(sigma_color), F(sigma_depth)
        c = scale * color
        demod = bool(demodulate) and albedo is not None
        if demod:
            albedo = np.asarray(albedo, F)
            a = np.where(albedo >= F(1e-3), albedo, F(1e-3)).astype(F)
            c = c / a
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
            sc = sigma_color * F(2.0 ** -i)
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            centre_bad = ~_finite3(c)
            lp = _lum(c)
            for dy, dx in itertools.product(range(-2, 3), range(-2, 3)):
                cq, inside = _shift(c, s * dx, s * dy)
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
                        xc = np.where(centre_bad, F(0), np.abs(lp - _lum(cq)) / sc).astype(F)
                    t = -(xz.astype(np.float64) + xc.astype(np.float64))
                    e = np.full((H, W), np.nan, F)
                    e[t < -200.0] = 0.0
                    m = (t >= -200.0) & (t <= 0.0)
                    e[m] = exp_small(t[m]).astype(F)
                    w = (h * wn) * e
                    take &= ~np.isnan(w)
                assert w.dtype == F and cq.dtype == F
                # (a skipped tap adds nothing: the sums below keep the tap order for every pixel on its own)
                acc = np.where(take[..., None], acc + w[..., None] * cq, acc)
                wsum = np.where(take, wsum + w, wsum)
            ok = wsum > 0
            c = np.where(ok[..., None], acc / np.where(ok, wsum, F(1))[..., None], c).astype(F)
        return (c * a if demod else c).astype(F)


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
class Params(C.Structure):          # include/art_hip.h ArtDenoiseParams (its own mirror: the host library needs no package)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("demodulate", C.c_int32),
                ("normal_log2", C.c_int32), ("variant", C.c_int32), ("scale", C.c_float), ("sigma_color", C.c_float), ("sigma_depth", C.c_float)]


_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "denoise_host")])
        L = C.CDLL(os.path.join(HERE, "denoise_host", "libdenoise_host.so"))
        L.dh_denoise.argtypes = [C.POINTER(Params)] + [C.c_void_p] * 5
        L.dh_denoise.restype = C.c_int
        _host = L
    return _host


def denoise_host(color, albedo=None, normal=None, depth=None, iterations=5, scale=1.0, sigma_color=4.0, sigma_depth=1.0, normal_log2=7,
                 demodulate=True):
    """the same call through csrc/art_denoise.h compiled by g++"""
    arrs = [None if x is None else np.ascontiguousarray(x, F) for x in (color, albedo, normal, depth)]
    H, W = arrs[0].shape[:2]
    out = np.zeros((H, W, 3), F)
    p = Params(W, H, iterations, 1 if demodulate else 0, normal_log2, 0, scale, sigma_color, sigma_depth)
    rc = host_lib().dh_denoise(C.byref(p), *[None if x is None else x.ctypes.data for x in arrs], out.ctypes.data)
    if rc:
        raise RuntimeError("dh_denoise refused its arguments")
    return out


def differ(a, b):
    """number of words that differ under the rule of devkat.same_words: both NaN, or the same bits"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return int((~ok).sum())


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
def planes(W, H, seed=0):
    """colours log-uniform over 1e-3 .. 1e3 with some exact zeros; unit normals with a block of zero vectors (the feature buffers' miss);
    positive depths on a slope with noise, with zeros; albedos in 0 .. 1 with zeros (below the floor)"""
    rng = np.random.default_rng(1000 * W + H + seed)
    color = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (H, W, 3))).astype(F)
    color[rng.random((H, W)) < 0.1] = 0.0
    n = rng.normal(size=(H, W, 3)) * 0.3 + np.array([0.0, 0.0, 1.0])
    n[:, W // 2:] = rng.normal(size=(H, W - W // 2, 3)) * 0.3 + np.array([1.0, 0.0, 0.0])
    normal = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    normal[: max(1, H // 3), : max(1, W // 4)] = 0.0
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (5.0 + 0.1 * xx + 0.05 * yy + rng.random((H, W)) * 0.2).astype(F)
    depth[: max(1, H // 3), : max(1, W // 4)] = 0.0
    albedo = rng.random((H, W, 3)).astype(F)
    albedo[rng.random((H, W)) < 0.1] = 0.0
    return color, albedo, normal, depth


SIZES = [(1, 1), (1, 9), (9, 1), (7, 5), (37, 23)]          # (W, H)


def combos():
    """(iterations, guides subset, demodulate, sigma_color, normal_log2): the full cross product, 192 of them"""
    subsets = [tuple(g for g, on in zip(("albedo", "normal", "depth"), bits) if on) for bits in itertools.product((0, 1), repeat=3)]
    return list(itertools.product((1, 2, 5), subsets, (0, 1), (0.0, 4.0), (0, 7)))


def combo_id(c):
    return "i%d-%s-d%d-sc%g-n%d" % (c[0], "".join(g[0] for g in c[1]) or "none", c[2], c[3], c[4])


def combo_args(pl, c):
    """planes() and one of combos() -> (color, dict of the guides given, dict of the parameters)"""
    color, albedo, normal, depth = pl
    it, sub, dm, sc, nl = c
    kw = dict(iterations=it, demodulate=bool(dm), sigma_color=sc, normal_log2=nl, scale=0.25, sigma_depth=1.0)
    g = dict(albedo=albedo if "albedo" in sub else None, normal=normal if "normal" in sub else None, depth=depth if "depth" in sub else None)
    return color, g, kw
