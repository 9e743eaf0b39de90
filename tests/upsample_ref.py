"""Reference of art_upsample_device written from the header comment of include/art_hip.h alone: plain numpy, binary32 arrays over the hi
pixels, Python loops over the 4 or 16 taps (exp_small is tests/denoise_ref.py's transcription of the header's).  Also the runner of
tests/upsample_host/upsample_host -- the product's text (csrc/art_upsample.h) compiled by g++ as a stand-alone program -- and the shapes,
planes and cases the tests of the call share."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from denoise_ref import exp_small

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
U32 = np.uint32
GUIDES = ("albedo", "normal", "depth", "id")


def amax(a, b):
    return np.where(a >= b, a, b).astype(F)


def axis(n, ln, jitter):
    """the mapping of one axis: (i0 [n] int64, fraction [n] float32, ratio float32)"""
    k = np.arange(n).astype(F)
    s = F(ln) / F(n)
    u = (k + F(0.5)) * s - (F(0.5) + F(jitter))
    fl = np.floor(u)
    assert u.dtype == F and fl.dtype == F
    return fl.astype(np.int64), (u - fl).astype(F), s


def kernel(footprint, a, f):
    if footprint == 2:
        return (F(1) - f).astype(F) if a == 0 else f
    return amax(F(0), F(1) - np.abs(F(a) - f) / F(2))


def taps(footprint):
    return range(0, 2) if footprint == 2 else range(-1, 3)


def upsample(lo_color, lo=None, hi=None, size=None, footprint=2, scale=1.0, sigma_depth=1.0, normal_log2=5, jitter=(0.0, 0.0), demodulate=True):
    """lo_color [LH, LW, 3]; lo, hi: dicts of the guides given (albedo, normal [.., .., 3], depth [.., ..] float32, id [.., ..] int32);
    size = (W, H) of the hi frame (needed only without a hi guide) -> (out [H, W, 3] float32, fallback [H, W] uint8)"""
    with np.errstate(all="ignore"):
        lo = {k: v for k, v in (lo or {}).items() if v is not None and k in GUIDES}
        hi = {k: v for k, v in (hi or {}).items() if v is not None and k in GUIDES}
        assert sorted(lo) == sorted(hi)
        lo_color = np.asarray(lo_color, F)
        LH, LW = lo_color.shape[:2]
        W, H = size if size is not None else next(iter(hi.values())).shape[1::-1]
        scale, sigma_depth = F(scale), F(sigma_depth)
        demod = bool(demodulate) and "albedo" in lo
        c = scale * lo_color
        if demod:
            c = c / amax(np.asarray(lo["albedo"], F), F(1e-3))
        assert c.dtype == F
        bad_colour = ~np.isfinite(c).all(axis=-1)
        bad_guides = np.zeros((LH, LW), bool)
        has_n, has_z, has_id = "normal" in lo, "depth" in lo, "id" in lo
        bad_p = np.zeros((H, W), bool)
        if has_n:
            n_lo, n_p = np.asarray(lo["normal"], F), np.asarray(hi["normal"], F)
            bad_guides |= ~np.isfinite(n_lo).all(axis=-1)
            bad_p |= ~np.isfinite(n_p).all(axis=-1)
        use_depth = has_z and sigma_depth > 0
        if has_z:
            z_lo, z = np.asarray(lo["depth"], F), np.asarray(hi["depth"], F)
            bad_guides |= ~np.isfinite(z_lo)
            bad_p |= ~np.isfinite(z)
            xi, yi = np.arange(W), np.arange(H)
            gx = F(0.5) * (z[:, np.minimum(xi + 1, W - 1)] - z[:, np.maximum(xi - 1, 0)])
            gy = F(0.5) * (z[np.minimum(yi + 1, H - 1), :] - z[np.maximum(yi - 1, 0), :])
            zfloor = F(1e-3) * z + F(1e-6)
        background = (has_n & ~bad_p & (n_p == 0).all(axis=-1)) if has_n else np.zeros((H, W), bool)
        i0, fx, sx = axis(W, LW, jitter[0])
        j0, fy, sy = axis(H, LH, jitter[1])
        acc, wsum = np.zeros((H, W, 3), F), np.zeros((H, W), F)
        acc2, wsum2 = np.zeros((H, W, 3), F), np.zeros((H, W), F)
        for b in taps(footprint):
            qy = np.clip(j0 + b, 0, LH - 1)[:, None]
            ky, oy = kernel(footprint, b, fy)[:, None], ((F(b) - fy) / sy)[:, None]
            for a in taps(footprint):
                qx = np.clip(i0 + a, 0, LW - 1)[None, :]
                h = (ky * kernel(footprint, a, fx)[None, :]).astype(F)
                ox = ((F(a) - fx) / sx)[None, :]
                cq, bcq = c[qy, qx], bad_colour[qy, qx]
                take = ~bad_p & ~bcq & ~bad_guides[qy, qx]
                if has_id:
                    take &= np.asarray(lo["id"])[qy, qx] == np.asarray(hi["id"])
                wn = np.ones((H, W), F)
                if has_n:
                    nq = n_lo[qy, qx]
                    d = (n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1]) + n_p[..., 2] * nq[..., 2]
                    wn = amax(d, F(0))
                    for _ in range(normal_log2):
                        wn = wn * wn
                xz = np.zeros((H, W), F)
                if use_depth:
                    xz = np.abs(z - z_lo[qy, qx]) / (sigma_depth * (np.abs(gx * ox) + np.abs(gy * oy)) + zfloor)
                assert xz.dtype == F and wn.dtype == F and h.dtype == F
                t = -(xz.astype(np.float64) + 0.0)
                e = np.full((H, W), np.nan, F)
                e[t < -200.0] = 0.0
                m = (t >= -200.0) & (t <= 0.0)
                e[m] = exp_small(t[m]).astype(F)
                w = (h * wn) * e
                if has_n:
                    take &= np.where(background, (nq == 0).all(axis=-1), ~np.isnan(w))
                    w = np.where(background, h, w).astype(F)
                else:
                    take &= ~np.isnan(w)
                # (a skipped tap adds nothing: the sums keep the tap order for every pixel on its own)
                acc = np.where(take[..., None], acc + w[..., None] * cq, acc)
                wsum = np.where(take, wsum + w, wsum)
                acc2 = np.where(~bcq[..., None], acc2 + h[..., None] * cq, acc2)
                wsum2 = np.where(~bcq, wsum2 + h, wsum2)
        assert acc.dtype == F and wsum.dtype == F and acc2.dtype == F and wsum2.dtype == F
        ok, ok2 = wsum > 0, wsum2 > 0
        out = np.where(ok[..., None], acc / wsum[..., None], np.where(ok2[..., None], acc2 / wsum2[..., None], F(0))).astype(F)
        fallback = np.where(ok, 0, np.where(ok2, 1, 2)).astype(np.uint8)
        if demod:
            out = out * amax(np.asarray(hi["albedo"], F), F(1e-3))
        return out.astype(F), fallback


def differ(a, b):
    """number of 32-bit words (or bytes) that differ"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, (a.shape, b.shape)
    v = U32 if a.dtype.itemsize == 4 else np.uint8
    return int((a.view(v) != b.view(v)).sum())


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
_built = False


def host_program():
    global _built
    d = os.path.join(HERE, "upsample_host")
    if not _built:
        subprocess.check_call(["make", "-s", "-C", d, "upsample_host"])
        _built = True
    return os.path.join(d, "upsample_host")


def _record(lo_color, lo, hi, size, footprint, scale, sigma_depth, normal_log2, jitter, demodulate):
    lo = {k: v for k, v in (lo or {}).items() if v is not None and k in GUIDES}
    hi = {k: v for k, v in (hi or {}).items() if v is not None and k in GUIDES}
    lo_color = np.ascontiguousarray(lo_color, F)
    LH, LW = lo_color.shape[:2]
    W, H = size if size is not None else next(iter(hi.values())).shape[1::-1]
    given = sum(1 << k for k, g in enumerate(GUIDES) if g in lo)
    parts = [struct.pack("<7i4fi", W, H, LW, LH, footprint, 1 if (demodulate and "albedo" in lo) else 0, normal_log2, scale, sigma_depth, jitter[0], jitter[1], given),
             lo_color.tobytes()]
    for g in GUIDES:
        if g in lo:
            dt = np.int32 if g == "id" else F
            parts += [np.ascontiguousarray(lo[g], dt).tobytes(), np.ascontiguousarray(hi[g], dt).tobytes()]
    return (W, H), b"".join(parts)


def upsample_host_many(calls):
    """upsample() for every dict of keyword arguments in `calls`, through csrc/art_upsample.h compiled by g++ (ONE run of the stand-alone
    program: IN holds the calls one after the other, OUT their outputs)"""
    sizes, blobs = zip(*[_record(**dict(dict(lo=None, hi=None, size=None, footprint=2, scale=1.0, sigma_depth=1.0, normal_log2=5, jitter=(0.0, 0.0),
                                             demodulate=True), **kw)) for kw in calls])
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(b"".join(blobs))
        subprocess.check_call([host_program(), "run", fin, fout])
        raw = np.fromfile(fout, np.uint8)
    res, at = [], 0
    for W, H in sizes:
        n = W * H
        res.append((raw[at:at + 12 * n].view(F).reshape(H, W, 3).copy(), raw[at + 12 * n:at + 13 * n].reshape(H, W).copy()))
        at += 13 * n
    assert at == raw.size
    return res


def upsample_host(lo_color, **kw):
    return upsample_host_many([dict(kw, lo_color=lo_color)])[0]


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
# (W, H, LW, LH, jitter): one pixel; every tap clamped; non-integer ratios that differ per axis; one pixel past a 16 x 16 tile and a wave,
# with jitter; tile edges in both axes at a ratio about 3; equal sizes; the ratio 2
SHAPES = [(1, 1, 1, 1, (0.0, 0.0)), (2, 2, 1, 1, (0.0, 0.0)), (13, 7, 5, 3, (0.0, 0.0)), (33, 17, 16, 8, (0.25, -0.375)), (70, 66, 23, 22, (0.0, 0.0)),
          (40, 24, 40, 24, (0.0, 0.0)), (48, 48, 24, 24, (0.0, 0.0))]
SHAPE_IDS = lambda s: "%dx%d_from_%dx%d" % s[:4]
ID_A, ID_B, ID_MISS, ID_ALONE = 3, 11, -1, 77


def region(u, v):
    """the synthetic scene over [0, 1)^2: (id, normal, depth).  Two surfaces either side of a slanted id boundary, with a depth step
    there; a normal crease across the first at v = 0.5; a block of background (a miss: id -1, zero normal, depth 0) in a corner"""
    first = u + 0.2 * v < 0.55
    miss = (u > 0.7) & (v < 0.35)
    ident = np.where(miss, ID_MISS, np.where(first, ID_A, ID_B)).astype(np.int32)
    n = np.where(first[..., None], np.where((v < 0.5)[..., None], [0.0, 0.0, 1.0], [0.0, 0.6, 0.8]), [0.8, 0.0, 0.6])
    n = np.where(miss[..., None], 0.0, n).astype(F)
    z = np.where(miss, 0.0, np.where(first, 5.0 + 2.0 * u + v, 9.0 + u)).astype(F)
    return ident, n, z


def centres(w, h):
    v, u = np.mgrid[0:h, 0:w]
    return (u + 0.5) / w, (v + 0.5) / h


def clean_planes(W, H, LW, LH, seed=0):
    """(lo_color, lo guides, hi guides) of the synthetic scene with nothing planted: finite colours and albedos, exact guides"""
    rng = np.random.default_rng(7919 * W + 131 * H + 17 * LW + LH + seed)
    lo_color = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), (LH, LW, 3))).astype(F)
    sides = {}
    for name, (w, h) in (("lo", (LW, LH)), ("hi", (W, H))):
        ident, n, z = region(*centres(w, h))
        albedo = np.where((ident == ID_MISS)[..., None], 0.0, rng.uniform(0.05, 1.0, (h, w, 3))).astype(F)
        sides[name] = dict(albedo=albedo, normal=n, depth=z, id=ident)
    return lo_color, sides["lo"], sides["hi"]


def planes(W, H, LW, LH, seed=0):
    """clean_planes() with the values the header's rules are about planted where the frames have room (15 lo pixels at least): NaN,
    infinite and negative lo colours; zero, negative and NaN lo albedos; NaN and infinite lo guides and a negative lo depth; NaN and
    infinite hi guides, a NaN and a negative hi albedo; a corner block of lo pixels without a finite colour (fallback 2 for the hi
    pixels whose every tap is clamped into it) and a hi pixel whose id no lo pixel has (fallback 1)"""
    lo_color, lo, hi = clean_planes(W, H, LW, LH, seed)
    if LW * LH < 15:
        return lo_color, lo, hi
    k = 3 if (LW >= 16 and LH >= 8) else 2
    lo_color[:k, :k] = np.nan
    lo_color[0, 0, 1] = np.inf
    lo_color[LH - 1, LW // 2] = (np.inf, 1.0, 1.0)
    lo_color[LH // 2, LW - 1] = (-1.0, -2.0, 0.5)
    lo_color[LH - 1, 0] = 0.0
    lo["albedo"][LH // 2, LW // 2] = (0.0, -1.0, np.nan)
    lo["normal"][LH - 1, 1] = (np.nan, 0.0, 1.0)
    lo["normal"][LH // 2, 1] = (0.0, np.inf, 0.0)
    lo["depth"][LH - 1, LW - 1] = np.inf
    lo["depth"][LH - 2, LW - 1] = np.nan
    lo["depth"][LH // 2, 0] = -3.0
    hi["normal"][H - 1, W // 2] = (0.0, np.nan, 1.0)
    hi["normal"][H // 2, 0] = (np.inf, 0.0, 0.0)
    hi["depth"][H - 1, W // 3] = np.nan
    hi["depth"][H // 2, W - 1] = np.inf
    hi["depth"][H // 2, W // 3] = -2.0
    hi["albedo"][H // 3, W // 2] = (np.nan, -1.0, 0.5)
    hi["id"][H - 2, 1] = ID_ALONE
    return lo_color, lo, hi


def subset(g, names):
    return {k: g[k] for k in names}


def cases(shape):
    """(name, keyword arguments of upsample()) at one shape: both footprints x {no guide, each guide alone, all}, with and without
    demodulation, sigma_depth <= 0, normal_log2 0 and 7"""
    W, H, LW, LH, jitter = shape
    lo_color, lo, hi = planes(W, H, LW, LH)
    out = []
    for fp in (2, 4):
        base = dict(lo_color=lo_color, footprint=fp, jitter=jitter, scale=0.25)
        for name, names, kw in (("none", (), dict(size=(W, H), demodulate=False)),
                                ("albedo_demod", ("albedo",), dict(demodulate=True)),
                                ("albedo_plain", ("albedo",), dict(demodulate=False)),
                                ("normal_log2_7", ("normal",), dict(normal_log2=7)),
                                ("normal_log2_0", ("normal",), dict(normal_log2=0)),
                                ("depth", ("depth",), dict(sigma_depth=1.0)),
                                ("depth_sigma_0", ("depth",), dict(sigma_depth=0.0)),
                                ("id", ("id",), dict()),
                                ("all_demod", GUIDES, dict(demodulate=True, normal_log2=7, sigma_depth=1.0)),
                                ("all_plain_sigma_negative", GUIDES, dict(demodulate=False, normal_log2=0, sigma_depth=-1.0)),
                                ("all_defaults", GUIDES, dict(sigma_depth=0.5))):
            out.append(("fp%d_%s" % (fp, name), dict(base, lo=subset(lo, names), hi=subset(hi, names), **kw)))
    return out


_refs = {}


def reference_results(shape):
    """[(name, kw, (out, fallback))] of cases(shape) by the numpy reference, computed once per process"""
    if shape not in _refs:
        _refs[shape] = [(name, kw, upsample(**kw)) for name, kw in cases(shape)]
    return _refs[shape]

