"""Reference of art_svgf_spatial_variance_device written from the header comment of include/art_hip.h alone: plain numpy over the pixels,
binary32 arrays except where the header names binary64, a Python loop over the taps of the window.  Also the runner of
tests/svgf_spatial_host/svgf_spatial_host -- the product's per-pixel text (csrc/art_svgf_spatial.h) compiled by g++ as a stand-alone
program -- and the synthetic histories and cases the tests of the call share."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from denoise_ref import F, _shift, exp_small

HERE = os.path.dirname(os.path.abspath(__file__))
U32 = np.uint32
QNAN = np.array([0x7fc00000], U32).view(F)[0]
INF = F(np.inf)


def spatial(hist, variance, radius=3, min_history=4.0, sigma_depth=1.0, normal_log2=7):
    """hist [3, H, W, 4], variance [H, W] float32 -> variance_out [H, W] float32"""
    with np.errstate(all="ignore"):
        hist = np.asarray(hist, F)
        H, W = hist.shape[1:3]
        variance = np.asarray(variance, F).reshape(H, W)
        min_history, sigma_depth = F(min_history), F(sigma_depth)
        n, m1, m2, z, N = hist[0, ..., 3], hist[1, ..., 0], hist[1, ..., 1], hist[1, ..., 2], hist[2, ..., :3]
        long_ = (n >= min_history) & np.isfinite(variance)
        use_depth = sigma_depth > 0
        gx, gy = np.zeros((H, W), F), np.zeros((H, W), F)
        if use_depth:
            xi, yi = np.arange(W), np.arange(H)
            gx = F(0.5) * (z[:, np.minimum(xi + 1, W - 1)] - z[:, np.maximum(xi - 1, 0)])
            gy = F(0.5) * (z[np.minimum(yi + 1, H - 1), :] - z[np.maximum(yi - 1, 0), :])
        zfloor = F(1e-3) * z + F(1e-6)
        ok = np.isfinite(n) & (n > 0) & np.isfinite(m1) & np.isfinite(m2) & np.isfinite(z) & np.isfinite(N).all(-1)
        Ns, S1, S2 = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                okq, inside = _shift(ok, dx, dy, fill=False)
                nq, m1q, m2q, zq, Nq = [_shift(a, dx, dy)[0] for a in (n, m1, m2, z, N)]
                take = inside & okq
                if dx == 0 and dy == 0:
                    w = np.ones((H, W), F)
                else:
                    d = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    wn = np.where(d >= F(0), d, F(0)).astype(F)
                    for _ in range(normal_log2):
                        wn = wn * wn
                    xz = np.zeros((H, W), F)
                    if use_depth:
                        xz = np.abs(z - zq) / (sigma_depth * (np.abs(gx * F(dx)) + np.abs(gy * F(dy))) + zfloor)
                    t = -xz.astype(np.float64)
                    e = np.full((H, W), np.nan, F)
                    e[t < -200.0] = 0.0
                    m = (t >= -200.0) & (t <= 0.0)
                    e[m] = exp_small(t[m]).astype(F)
                    w = wn * e
                    take &= ~np.isnan(w)
                assert w.dtype == F
                k = w.astype(np.float64) * nq.astype(np.float64)
                Ns = np.where(take, Ns + k, Ns)
                S1 = np.where(take, S1 + k * m1q.astype(np.float64), S1)
                S2 = np.where(take, S2 + k * m2q.astype(np.float64), S2)
        M1, M2 = S1 / Ns, S2 / Ns
        D = M2 - M1 * M1
        D0 = np.where(D < 0.0, 0.0, D)
        v = ((D0 * (Ns / (Ns - 1.0))) / n.astype(np.float64)).astype(F)
        v = np.where(np.isnan(v), QNAN, v)
        v = np.where(Ns < 2.0, INF, v)
        out = np.where(long_, variance, v).astype(F)
        return out


def differ(a, b):
    """number of words that differ, bit for bit (a NaN must be the header's quiet NaN on both sides)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return int((a.view(U32) != b.view(U32)).sum())


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
_built = False


def host_program():
    global _built
    d = os.path.join(HERE, "svgf_spatial_host")
    if not _built:
        subprocess.check_call(["make", "-s", "-C", d, "svgf_spatial_host"])
        _built = True
    return os.path.join(d, "svgf_spatial_host")


def spatial_host(hist, variance, radius=3, min_history=4.0, sigma_depth=1.0, normal_log2=7, in_place=False):
    """the same call through csrc/art_svgf_spatial.h compiled by g++ (a stand-alone program: IN and OUT are files)"""
    hist = np.ascontiguousarray(hist, F)
    H, W = hist.shape[1:3]
    variance = np.ascontiguousarray(variance, F).reshape(H, W)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<4i2f", W, H, radius, normal_log2, min_history, sigma_depth))
            f.write(hist.tobytes()); f.write(variance.tobytes())
        subprocess.check_call([host_program(), fin, fout] + (["inplace"] if in_place else []))
        return np.fromfile(fout, F).reshape(H, W)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (5, 3), (37, 29)]          # (W, H): one pixel, smaller than a window, no multiple of any tile
RADII = (1, 2, 3)


def temporal_variance(n, m1, m2):
    """step 6 of art_temporal_device's arithmetic (the plane a history arrives with)"""
    with np.errstate(all="ignore"):
        n64, d1 = n.astype(np.float64), m1.astype(np.float64)
        D = m2.astype(np.float64) - d1 * d1
        D0 = np.where(D < 0.0, 0.0, D)
        return np.where(n < 2, INF, ((D0 * (n64 / (n64 - 1.0))) / n64).astype(F)).astype(F)


def history(W, H, n, seed=0):
    """a synthetic history with lengths n ([H, W] or a scalar): a slanted floor (depth grows to the right and downwards), over the right
    third a panel 4 nearer with a tilted normal (a depth step and a normal change inside every window that straddles its edge), and a
    strip at the bottom whose normal is flipped.  Returns (hist [3, H, W, 4], variance [H, W]) as art_temporal_device would leave them."""
    rng = np.random.default_rng(7919 * W + 31 * H + seed)
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = 10.0 + 0.05 * X + 0.02 * Y
    pan = X >= (2 * W) // 3 if W >= 3 else np.zeros((H, W), bool)
    z = np.where(pan, z - 4.0, z)
    nrm = np.zeros((H, W, 3), F)
    nrm[...] = (0.0, 0.0, 1.0)
    nrm[pan] = np.array([0.6, 0.0, 0.8], F)
    if H >= 4:
        nrm[H - max(1, H // 5):] *= F(-1)
    lum = rng.uniform(0.2, 2.0, (H, W))
    rel = np.exp(rng.uniform(np.log(1e-2), np.log(2.0), (H, W)))
    h = np.zeros((3, H, W, 4), F)
    h[0, ..., :3] = lum[..., None].astype(F)
    h[0, ..., 3] = np.broadcast_to(np.asarray(n, F), (H, W))
    h[1, ..., 0] = lum.astype(F); h[1, ..., 1] = (lum * lum * (1.0 + rel * rel)).astype(F); h[1, ..., 2] = z.astype(F)
    h.view(np.int32)[1, ..., 3] = np.where(pan, 2, 1)
    h[2, ..., :3] = nrm
    return h, temporal_variance(h[0, ..., 3], h[1, ..., 0], h[1, ..., 1])


def spots(H, W, k):
    """k-th of a few pixel positions spread over the frame"""
    return ((k * 5 + 1) % H, (k * 7 + 2) % W)


def cases(W, H):
    """(name, keyword arguments of spatial()) at one frame size; every radius is run over each by the tests"""
    X, Y = np.meshgrid(np.arange(W), np.arange(H))
    out = []

    def add(name, n, edit=None, seed=0, **kw):
        h, v = history(W, H, n, seed)
        if edit:
            edit(h, v)
        out.append((name, dict(dict(hist=h, variance=v, min_history=4.0, sigma_depth=1.0, normal_log2=7), **kw)))

    add("all_short", 1.0)
    add("all_short_two_colours", 2.0, seed=1)
    add("all_long", 8.0)
    add("checkerboard", np.where((X + Y) % 2 == 0, 1.0, 8.0))
    one = np.full((H, W), 8.0); one[spots(H, W, 3)] = 1.0
    add("single_short_pixel", one)
    add("blocks_of_waves", np.where((Y // 4) % 2 == 0, 8.0, 1.0))           # whole 16 x 4 strips long, whole strips short
    zeros = np.where((X + 2 * Y) % 3 == 0, 0.0, 1.0); zeros[spots(H, W, 1)] = -1.0
    add("n_zero_taps", zeros)

    def e_bad(h, v):
        k = 0
        for plane, word in ((0, 3), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)):
            for bad in (np.nan, np.inf, -np.inf):
                h[plane][spots(H, W, k)][word] = bad
                k += 1
    add("bad_words_short", 1.0, edit=e_bad)
    add("bad_words_mixed", np.where((X + Y) % 2 == 0, 2.0, 8.0), edit=e_bad, seed=2)

    def e_var(h, v):
        v[spots(H, W, 0)] = np.inf; v[spots(H, W, 2)] = np.nan; v[spots(H, W, 4)] = -np.inf
    add("variance_in_not_finite_at_long_pixels", 8.0, edit=e_var)

    def e_step(h, v):
        h[1, :, W // 2:, 2] += F(25.0); h[2, H // 2:, :, :3] *= F(-1)
    add("depth_step_and_normal_flip", 1.0, edit=e_step, seed=3)
    add("sigma_depth_zero", 1.0, sigma_depth=0.0)
    add("sigma_depth_negative", np.where((X + Y) % 2 == 0, 1.0, 8.0), sigma_depth=-1.0)
    add("sigma_depth_small_normal_log2_0", 1.0, sigma_depth=0.05, normal_log2=0, seed=4)
    add("min_history_infinite", 8.0, min_history=np.inf)
    add("min_history_zero", 1.0, min_history=0.0)

    def e_neg(h, v):
        h[1][spots(H, W, 0)][2] = -3.0; h[1][spots(H, W, 1)][2] = 0.0
    add("negative_and_zero_depth", 1.0, edit=e_neg, seed=5)
    return out
