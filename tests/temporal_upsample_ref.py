"""Reference of art_temporal_upsample_device written from the header comment of include/art_hip.h alone: plain numpy, binary32 arrays over
the hi pixels except where the header names binary64, Python loops over the four lo taps and the four history taps.  Also the runner of
tests/temporal_upsample_host/temporal_upsample_host -- the product's text (csrc/art_temporal_upsample.h) compiled by g++ as a stand-alone
program -- and the shapes, planes and cases the tests of the call share."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import temporal_ref as T
from temporal_ref import F, I32, _dot, _finite3, _rows, camera
from upsample_ref import axis, differ      # noqa: F401 (differ: for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
GUIDES = ("normal", "depth", "id")
BRANCHES = ("history_and_samples", "history_alone", "samples_alone", "unguided", "nothing")      # step C, in the header's order


def amax(a, b):
    return np.where(a >= b, a, b).astype(F)


def _history(cur, cam_prev, hist, W, H, z, pid, N, has_depth, has_normal, has_id, motion, depth_tol, normal_min):
    """steps 2 to 4 of art_temporal_device on the hi guides (with motion: art_temporal_motion_device's step 3): (has [H, W] bool, the six
    fields hist.r, g, b, n, m1, m2 divided by wsum where has)"""
    own = np.full((H, W), hist is None)
    if has_depth:
        own |= ~((z > 0) & np.isfinite(z))
    if has_normal:
        own |= ~_finite3(N)
    sums = [np.zeros((H, W), F) for _ in range(6)]
    wsum = np.zeros((H, W), F)
    if hist is not None:
        hist = np.asarray(hist, F)
        Hp, Wp = hist.shape[1:3]
        prev = camera(cam_prev, Wp, Hp)
        assert prev is not None
        X, Y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
        ok = ~own
        same = cur["words"] == prev["words"]
        if not has_depth or (same and motion is None):
            fx, fy, e = X + F(0.5), Y + F(0.5), z
        else:
            rx, ry = (X + F(0.5)) - F(W) / F(2), (Y + F(0.5)) - F(H) / F(2)
            rz = np.full((H, W), cur["cam_z"], F)
            li = F(1) / np.sqrt(_dot(rx, ry, rz, rx, ry, rz))
            t = _rows(cur["M"], li * rx, li * ry, li * rz)
            lj = F(1) / np.sqrt(_dot(*t, *t))
            d = [lj * t[k] for k in range(3)]
            if motion is not None:
                ok &= np.isfinite(motion).all(-1)
                v = [((cur["pos"][k] + z * d[k]) + motion[..., k]) - prev["pos"][k] for k in range(3)]
            else:
                v = [(cur["pos"][k] + z * d[k]) - prev["pos"][k] for k in range(3)]
            e = np.sqrt(_dot(*v, *v))
            q = _rows(prev["I"], *v)
            ok &= q[2] * prev["cam_z"] > 0
            k = prev["cam_z"] / q[2]
            fx, fy = q[0] * k + F(Wp) / F(2), q[1] * k + F(Hp) / F(2)
        gx, gy = fx - F(0.5), fy - F(0.5)
        ok &= (gx > -1) & (gx < F(Wp)) & (gy > -1) & (gy < F(Hp))
        gx, gy = np.where(ok, gx, F(0)).astype(F), np.where(ok, gy, F(0)).astype(F)
        flx, fly = np.floor(gx), np.floor(gy)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        ax, ay = gx - flx, gy - fly
        assert ax.dtype == F and e.dtype == F
        for t in range(4):
            ddx, ddy = t & 1, t >> 1
            w = (ax if ddx else F(1) - ax) * (ay if ddy else F(1) - ay)
            qx, qy = ix + ddx, iy + ddy
            inside = (qx >= 0) & (qx < Wp) & (qy >= 0) & (qy < Hp)
            qx, qy = np.clip(qx, 0, Wp - 1), np.clip(qy, 0, Hp - 1)
            a, b, g = hist[0][qy, qx], hist[1][qy, qx], hist[2][qy, qx]
            cnt = ok & (w > 0) & inside & np.isfinite(a).all(-1) & (a[..., 3] > 0) & np.isfinite(b[..., :3]).all(-1) & _finite3(g[..., :3])
            if has_depth:
                cnt &= np.abs(b[..., 2] - e) <= depth_tol * e
            if has_normal:
                cnt &= _dot(N[..., 0], N[..., 1], N[..., 2], g[..., 0], g[..., 1], g[..., 2]) >= normal_min
            if has_id:
                cnt &= np.ascontiguousarray(b[..., 3]).view(I32) == pid
            fields = (a[..., 0], a[..., 1], a[..., 2], a[..., 3], b[..., 0], b[..., 1])
            assert w.dtype == F
            sums = [np.where(cnt, s + w * f, s).astype(F) for s, f in zip(sums, fields)]
            wsum = np.where(cnt, wsum + w, wsum).astype(F)
    has = wsum > 0
    one = np.where(has, wsum, F(1))
    return has, [(s / one).astype(F) for s in sums]


def temporal_upsample(lo_color, lo_moments, n_colours, cam_cur, cam_prev=None, hist=None, lo=None, hi=None, size=None, jitter=(0.0, 0.0), radius=1.0,
                      min_confidence=0.25, max_history=64, depth_tol=0.05, normal_min=0.9, scale=1.0, branches=False):
    """lo_color [LH, LW, 3], lo_moments [LH, LW, 2]; lo, hi: dicts of the guides given (normal [.., .., 3], depth [.., ..] float32, id
    [.., ..] int32; hi may hold motion [H, W, 3]); size = (W, H) of the hi frame (needed only without a hi plane); hist [3, Hp, Wp, 4] or
    None -> (hist_out [3, H, W, 4], out [H, W, 3], variance [H, W], length [H, W]) float32, fallback [H, W] uint8; with branches, a sixth:
    which line of step C each pixel took, as an index into BRANCHES"""
    with np.errstate(all="ignore"):
        lo = {k: v for k, v in (lo or {}).items() if v is not None and k in GUIDES}
        motion = (hi or {}).get("motion")
        hi = {k: v for k, v in (hi or {}).items() if v is not None and k in GUIDES}
        assert sorted(lo) == sorted(hi)
        lo_color = np.asarray(lo_color, F)
        LH, LW = lo_color.shape[:2]
        lo_moments = np.asarray(lo_moments, F).reshape(LH, LW, 2)
        if hi:
            H, W = next(iter(hi.values())).shape[:2]
        elif motion is not None:
            H, W = motion.shape[:2]
        else:
            W, H = size if size is not None else (LW, LH)
        if motion is not None:
            motion = np.asarray(motion, F).reshape(H, W, 3)
        cur = camera(cam_cur, W, H)
        assert cur is not None
        scale, depth_tol, normal_min, n_cur = F(scale), F(depth_tol), F(normal_min), F(n_colours)
        radius, minc, maxh = F(radius), F(min_confidence), F(max_history)
        has_n, has_z, has_id = "normal" in lo, "depth" in lo, "id" in lo
        # preparation of the lo pixels
        c = scale * lo_color
        m1, m2 = lo_moments[..., 0] / n_cur, lo_moments[..., 1] / n_cur
        val = np.concatenate([c, m1[..., None], m2[..., None]], -1).astype(F)          # the five values a tap carries
        bad_colour = ~np.isfinite(val).all(-1)
        bad_guides = np.zeros((LH, LW), bool)
        n_lo = np.asarray(lo["normal"], F) if has_n else np.zeros((LH, LW, 3), F)
        z_lo = np.asarray(lo["depth"], F) if has_z else np.zeros((LH, LW), F)
        id_lo = np.asarray(lo["id"], I32) if has_id else np.zeros((LH, LW), I32)
        if has_n:
            bad_guides |= ~_finite3(n_lo)
        if has_z:
            bad_guides |= ~np.isfinite(z_lo)
        # the hi pixel
        z = np.asarray(hi["depth"], F) if has_z else np.zeros((H, W), F)
        pid = np.asarray(hi["id"], I32) if has_id else np.zeros((H, W), I32)
        N = np.asarray(hi["normal"], F) if has_n else np.zeros((H, W, 3), F)
        bad = np.zeros((H, W), bool)
        if has_z:
            bad |= ~np.isfinite(z)
        if has_n:
            bad |= ~_finite3(N)
        miss = (~(z > 0)) if has_z else np.zeros((H, W), bool)
        # A. this frame
        i0, fx, sx = axis(W, LW, jitter[0])
        j0, fy, sy = axis(H, LH, jitter[1])
        K, Hs, Us = [np.zeros((H, W), F) for _ in range(3)]
        Ck, Ch, Cu = [np.zeros((H, W, 5), F) for _ in range(3)]
        for t in range(4):
            a, b = t & 1, t >> 1
            qx, qy = (i0 + a)[None, :], (j0 + b)[:, None]
            inside = (qx >= 0) & (qx < LW) & (qy >= 0) & (qy < LH)
            qx, qy = np.clip(qx, 0, LW - 1), np.clip(qy, 0, LH - 1)
            dx, dy = ((F(a) - fx) / sx)[None, :], ((F(b) - fy) / sy)[:, None]
            k = (amax(F(0), F(1) - np.abs(dx) / radius) * amax(F(0), F(1) - np.abs(dy) / radius)).astype(F)
            h = ((fx if a else F(1) - fx)[None, :] * (fy if b else F(1) - fy)[:, None]).astype(F)
            k, h = np.broadcast_to(k, (H, W)), np.broadcast_to(h, (H, W))
            v = val[qy, qx]
            usable = inside & ~bad_colour[qy, qx]
            cnt = usable & ~bad_guides[qy, qx] & ~bad
            if has_id:
                cnt &= id_lo[qy, qx] == pid
            hit_tests = np.ones((H, W), bool)
            if has_n:
                nq = n_lo[qy, qx]
                hit_tests &= _dot(N[..., 0], N[..., 1], N[..., 2], nq[..., 0], nq[..., 1], nq[..., 2]) >= normal_min
            if has_z:
                hit_tests &= np.abs(z_lo[qy, qx] - z) <= depth_tol * z
            cnt &= np.where(miss, ~(z_lo[qy, qx] > 0), hit_tests)
            for w, take, S, C in ((k, cnt & (k > 0), "K", Ck), (h, cnt & (h > 0), "Hs", Ch), (h, usable & (h > 0), "Us", Cu)):
                assert w.dtype == F and v.dtype == F
                C[...] = np.where(take[..., None], C + w[..., None] * v, C)
                if S == "K":
                    K = np.where(take, K + w, K).astype(F)
                elif S == "Hs":
                    Hs = np.where(take, Hs + w, Hs).astype(F)
                else:
                    Us = np.where(take, Us + w, Us).astype(F)
        kappa = np.where(K < 1, K, F(1)).astype(F)
        n_eff = kappa * n_cur
        # B. the history
        has, (hr, hg, hb, hn, hm1, hm2) = _history(cur, cam_prev, hist, W, H, z, pid, N, has_z, has_n, has_id, motion, depth_tol, normal_min)
        hv = np.stack([hr, hg, hb, hm1, hm2], -1)
        # C. combine
        def mean(C, S):
            return (C / np.where(S > 0, S, F(1))[..., None]).astype(F)
        branch = np.where(has, np.where(K > 0, 0, 1), np.where(Hs > 0, 2, np.where(Us > 0, 3, 4)))
        # history and K > 0
        cv = mean(Ck, K)
        cap = maxh - n_eff
        f = np.where(hn > cap, cap / np.where(has, hn, F(1)), F(1)).astype(F)
        n0 = n_eff + f * hn
        a0 = n_eff / n0
        b0 = F(1) - a0
        v0 = (a0[..., None] * cv + b0[..., None] * hv).astype(F)
        # history and K == 0
        f1 = np.where(hn > maxh, maxh / np.where(has, hn, F(1)), F(1)).astype(F)
        n1 = f1 * hn
        # no history
        n2 = n_cur * amax(kappa, minc)
        n3 = np.full((H, W), n_cur * minc, F)
        vals = [v0, hv, mean(Ch, Hs), mean(Cu, Us), np.zeros((H, W, 5), F)]
        ns = [n0, n1, n2, n3, np.zeros((H, W), F)]
        v = np.zeros((H, W, 5), F)
        n = np.zeros((H, W), F)
        for k in range(5):
            v = np.where((branch == k)[..., None], vals[k], v).astype(F)
            n = np.where(branch == k, ns[k], n).astype(F)
        fallback = np.where(branch == 3, 1, np.where(branch == 4, 2, 0)).astype(np.uint8)
        # D. the outputs
        out = np.zeros((3, H, W, 4), F)
        out[0, ..., :3] = v[..., :3]; out[0, ..., 3] = n
        out[1, ..., 0] = v[..., 3]; out[1, ..., 1] = v[..., 4]; out[1, ..., 2] = z
        out.view(I32)[1, ..., 3] = pid
        out[2, ..., :3] = N
        n64, d1 = n.astype(np.float64), v[..., 3].astype(np.float64)
        D = v[..., 4].astype(np.float64) - d1 * d1
        D0 = np.where(D < 0.0, 0.0, D)
        var = np.where(n < 2, F(np.inf), ((D0 * (n64 / (n64 - 1.0))) / n64).astype(F)).astype(F)
        res = (out, np.ascontiguousarray(v[..., :3]), var, n, fallback)
        return res + (branch,) if branches else res


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
_built = False
DEFAULTS = dict(cam_prev=None, hist=None, lo=None, hi=None, size=None, jitter=(0.0, 0.0), radius=1.0, min_confidence=0.25, max_history=64, depth_tol=0.05,
                normal_min=0.9, scale=1.0)


def host_program():
    global _built
    d = os.path.join(HERE, "temporal_upsample_host")
    if not _built:
        subprocess.check_call(["make", "-s", "-C", d, "temporal_upsample_host"])
        _built = True
    return os.path.join(d, "temporal_upsample_host")


def _cam_words(cam, w, h):
    return np.asarray(cam[0], F).reshape(3).tobytes() + np.asarray(cam[1], F).reshape(16).tobytes() + struct.pack("<2i", w, h)


def _record(lo_color, lo_moments, n_colours, cam_cur, cam_prev, hist, lo, hi, size, jitter, radius, min_confidence, max_history, depth_tol, normal_min, scale):
    lo = {k: v for k, v in (lo or {}).items() if v is not None and k in GUIDES}
    motion = (hi or {}).get("motion")
    hi = {k: v for k, v in (hi or {}).items() if v is not None and k in GUIDES}
    lo_color = np.ascontiguousarray(lo_color, F)
    LH, LW = lo_color.shape[:2]
    if hi:
        H, W = next(iter(hi.values())).shape[:2]
    elif motion is not None:
        H, W = motion.shape[:2]
    else:
        W, H = size if size is not None else (LW, LH)
    given = sum(1 << k for k, g in enumerate(GUIDES) if g in lo) | (8 if motion is not None else 0) | (16 if hist is not None else 0)
    prev = _cam_words(cam_prev, hist.shape[2], hist.shape[1]) if hist is not None else bytes(84)
    parts = [_cam_words(cam_cur, W, H), prev, struct.pack("<2i3f2i4f", n_colours, max_history, scale, depth_tol, normal_min, LW, LH, jitter[0], jitter[1], radius, min_confidence),
             struct.pack("<i", given), lo_color.tobytes(), np.ascontiguousarray(lo_moments, F).tobytes()]
    assert len(lo_moments.reshape(-1)) == 2 * LW * LH
    for g in GUIDES:
        if g in lo:
            dt = I32 if g == "id" else F
            parts += [np.ascontiguousarray(lo[g], dt).tobytes(), np.ascontiguousarray(hi[g], dt).tobytes()]
    if motion is not None:
        parts.append(np.ascontiguousarray(motion, F).tobytes())
    if hist is not None:
        parts.append(np.ascontiguousarray(hist, F).tobytes())
    return (W, H), b"".join(parts)


def temporal_upsample_host_many(calls):
    """temporal_upsample() for every dict of keyword arguments in `calls`, through csrc/art_temporal_upsample.h compiled by g++ (ONE run of
    the stand-alone program: IN holds the calls one after the other, OUT their outputs)"""
    sizes, blobs = zip(*[_record(**dict(DEFAULTS, **kw)) for kw in calls])
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(b"".join(blobs))
        subprocess.check_call([host_program(), "run", fin, fout])
        raw = np.fromfile(fout, np.uint8)
    res, at = [], 0
    for W, H in sizes:
        n = W * H
        cut = lambda nbytes: raw[at:at + nbytes]
        hist = cut(48 * n).view(F).reshape(3, H, W, 4).copy(); at += 48 * n
        out = cut(12 * n).view(F).reshape(H, W, 3).copy(); at += 12 * n
        var = cut(4 * n).view(F).reshape(H, W).copy(); at += 4 * n
        length = cut(4 * n).view(F).reshape(H, W).copy(); at += 4 * n
        fb = cut(n).reshape(H, W).copy(); at += n
        res.append((hist, out, var, length, fb))
    assert at == raw.size
    return res


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
# (W, H, LW, LH): one pixel; equal sizes; a non-integer ratio on few pixels; one pixel past a 16 x 16 tile in both axes at a ratio near
# 2; the ratio 2 over nine tiles; a ratio about 3 that differs per axis
SHAPES = [(1, 1, 1, 1), (5, 3, 5, 3), (7, 5, 4, 3), (17, 33, 9, 17), (48, 48, 24, 24), (70, 66, 23, 22)]
SHAPE_IDS = lambda s: "%dx%d_from_%dx%d" % s
NEAR = float(np.nextafter(F(0.5), F(0)))                      # the largest binary32 below 0.5
JITTERS = [(0.0, 0.0), (0.25, -0.375), (NEAR, -NEAR), (-NEAR, NEAR)]
NC = 2


def bound(W, H, LW, LH):
    """the largest legal radius"""
    return float(min(F(W) / F(LW), F(H) / F(LH)))


def lo_frame(camr, W, H, LW, LH, jitter, seed):
    """the lo frame of temporal_ref.frame's scene under camera camr with its grid moved by `jitter`: the planes at the sample positions the
    header's mapping gives a lo pixel (the hi frame's camera at LW x LH, sheared as the package's jittered_camera does)"""
    pos, m = camr
    m = np.array(m, np.float64).reshape(4, 4)
    m[:3, 2] = m[:3, 2] + (jitter[0] * m[:3, 0] + jitter[1] * m[:3, 1]) / -float(LW)
    # the hi camera spans W pixels with cam_z = -W; at LW pixels with cam_z = -LW the field of view is the same
    fr = T.frame((pos, m.astype(F)), LW, LH, seed=seed, n_colours=NC)
    return fr


def frames(W, H, LW, LH, camr, jitter, seed):
    """(lo_color, lo_moments, lo guides, hi guides) of one frame"""
    lf = lo_frame(camr, W, H, LW, LH, jitter, seed)
    hf = T.frame(camr, W, H, seed=seed + 50, n_colours=NC)
    lo = dict(normal=lf["normal"], depth=lf["depth"], id=lf["ids"])
    hi = dict(normal=hf["normal"], depth=hf["depth"], id=hf["ids"])
    return lf["color"], lf["moments"], lo, hi


def subset(g, names):
    return {k: g[k] for k in names if k in g}


def first_history(W, H, LW, LH, camr, frames_=2, **kw):
    """a hi history of the header's own making: `frames_` jittered frames at camera camr, from the reference"""
    h = None
    for k in range(frames_):
        j = JITTERS[(k + 1) % len(JITTERS)]
        lc, lm, lo, hi = frames(W, H, LW, LH, camr, j, 100 + k)
        h = temporal_upsample(lc, lm, NC, camr, camr, h, lo, hi, jitter=j, radius=min(1.0, bound(W, H, LW, LH)), scale=1.0 / NC, max_history=16, **kw)[0]
    return h


def plant(lc, lm, lo, hi, hist):
    """NaN, infinite and negative values in the lo colour, the lo moments, every guide of both sides and the history, where the frames
    have room (15 lo pixels at least)"""
    LH, LW = lc.shape[:2]
    H, W = hi["depth"].shape
    if LW * LH < 12:
        return
    lc[0, 0] = np.nan
    lc[LH - 1, LW // 2] = (np.inf, 1.0, 1.0)
    lc[LH // 2, LW - 1] = (-1.0, -2.0, 0.5)
    lm[LH - 1, 0, 0] = np.nan
    lm[0, LW - 1, 1] = np.inf
    lm[LH // 2, 0] = (-1.0, 2.0)
    lo["normal"][LH - 1, 1] = (np.nan, 0.0, 1.0)
    lo["normal"][LH // 2, 1] = (0.0, np.inf, 0.0)
    lo["depth"][LH - 1, LW - 1] = np.inf
    lo["depth"][LH - 2, LW - 1] = np.nan
    lo["depth"][LH // 2, LW // 2] = -3.0
    hi["normal"][H - 1, W // 2] = (0.0, np.nan, 1.0)
    hi["normal"][H // 2, 0] = (np.inf, 0.0, 0.0)
    hi["depth"][H - 1, W // 3] = np.nan
    hi["depth"][H // 2, W - 1] = np.inf
    hi["depth"][H // 2, W // 3] = -2.0
    hi["id"][H - 2, 1] = 77
    if hist is not None:
        Hp, Wp = hist.shape[1:3]
        hist[0, 0, Wp // 2, 0] = np.nan
        hist[0, Hp // 2, Wp // 3, 2] = -np.inf
        hist[1, Hp - 1, Wp - 1, 1] = np.nan
        hist[0, Hp // 3, 0, 3] = 0.0
        hist[0, Hp // 3, Wp - 1, 3] = -1.0
        hist[1, Hp // 2, Wp // 2, 2] = np.nan
        hist[2, 0, 0, 0] = np.inf
        hist[1, Hp - 1, 0, 0] = -4.0


def cases(shape):
    """(name, keyword arguments of temporal_upsample()) at one shape: the jitters, radius 1 and the upper bound, every guide alone, all and
    none, with and without history and motion, cameras equal, panned and with a previous frame of another size, planted values, hi
    misses over lo hits and the reverse, and a frame that takes all five lines of step C"""
    W, H, LW, LH = shape
    base, pan = T.cam(), T.cam((0.4, -0.1, 0.0))
    turned = T.cam(yaw=0.9)                       # part of the frame looks past the wall's horizon... and past the panel: misses
    top = bound(W, H, LW, LH)
    r1 = min(1.0, top)
    kw0 = dict(n_colours=NC, scale=1.0 / NC, max_history=16, depth_tol=0.05, normal_min=0.9, min_confidence=0.25)
    h_base = first_history(W, H, LW, LH, base)
    out = []

    def add(name, camr, jitter=(0.0, 0.0), prev=base, hist=h_base, names=GUIDES, radius=r1, seed=1, edit=None, motion=None, **over):
        lc, lm, lo, hi = frames(W, H, LW, LH, camr, jitter, seed)
        hist = None if hist is None else hist.copy()
        if edit:
            edit(lc, lm, lo, hi, hist)
        lo, hi = subset(lo, names), subset(hi, names)
        if motion is not None:
            hi["motion"] = motion
        out.append((name, dict(kw0, lo_color=lc, lo_moments=lm, cam_cur=camr, cam_prev=prev if hist is not None else None, hist=hist, lo=lo, hi=hi,
                               size=(W, H), jitter=jitter, radius=radius, **over)))

    for k, j in enumerate(JITTERS):
        add("jitter%d_first_frame" % k, base, j, hist=None)
        add("jitter%d_rest" % k, base, j)
        add("jitter%d_pan_radius_top" % k, pan, j, radius=top)
    add("radius_top_rest", base, JITTERS[1], radius=top)
    add("radius_small", base, JITTERS[1], radius=0.25 * r1)
    for g in GUIDES:
        add("only_" + g, pan, JITTERS[1], names=(g,))
        add("only_%s_first_frame" % g, pan, JITTERS[1], names=(g,), hist=None)
    add("no_guides", pan, JITTERS[1], names=())
    add("no_guides_first_frame", base, JITTERS[2], names=(), hist=None)
    add("prev_other_size", T.cam((0.1, 0.0, 0.0)), JITTERS[1], hist=first_history(W + 3, H + 2, LW + 1, LH + 1, base))
    add("capped", base, JITTERS[3], max_history=3)
    add("confidence_1", pan, JITTERS[1], min_confidence=1.0, hist=None)
    add("misses", turned, JITTERS[1], prev=T.cam(yaw=0.88), hist=first_history(W, H, LW, LH, T.cam(yaw=0.88)))
    add("planted_rest", base, JITTERS[1], edit=plant)
    add("planted_pan", pan, JITTERS[3], edit=plant, radius=top)
    add("planted_first_frame", base, JITTERS[2], edit=plant, hist=None)

    def swap_misses(lc, lm, lo, hi, hist):
        """a block of hi misses over lo hits, and a block of lo misses under hi hits"""
        hh, ww = max(1, H // 3), max(1, W // 3)
        hi["depth"][:hh, :ww] = 0.0; hi["normal"][:hh, :ww] = 0.0; hi["id"][:hh, :ww] = -1
        lh, lw = max(1, LH // 3), max(1, LW // 3)
        lo["depth"][LH - lh:, LW - lw:] = 0.0; lo["normal"][LH - lh:, LW - lw:] = 0.0; lo["id"][LH - lh:, LW - lw:] = -1
    add("hi_miss_over_lo_hit_and_reverse", base, JITTERS[1], edit=swap_misses)
    add("hi_miss_over_lo_hit_and_reverse_first_frame", base, JITTERS[1], edit=swap_misses, hist=None)
    add("hi_miss_depth_only", base, JITTERS[1], edit=swap_misses, names=("depth",))

    # motion: the plane that takes every hit pixel back by a shift in the previous frame of the same camera
    import temporal_motion_ref as TM
    for name, camr, shift in (("motion_zero_equal_cameras", base, (0.0, 0.0)), ("motion_fractional_equal_cameras", base, (0.37, 1.62)),
                              ("motion_moving_camera", T.cam((0.05, 0.01, 0.0), yaw=0.004), (-1.25, 0.5))):
        hf = T.frame(camr, W, H, seed=1 + 50, n_colours=NC)
        add(name, camr, JITTERS[1], motion=TM.pixel_shift(camr, hf, *shift))
    hf = T.frame(base, W, H, seed=1 + 50, n_colours=NC)
    mo = TM.pixel_shift(base, hf, 0.5, 0.0)
    mo.reshape(-1, 3)[0, 0] = np.nan; mo.reshape(-1, 3)[-1, 2] = np.inf
    add("motion_not_finite", base, JITTERS[1], motion=mo)
    add("motion_no_depth", base, JITTERS[1], motion=mo, names=("normal", "id"))
    add("motion_first_frame", base, JITTERS[1], motion=mo, hist=None)

    def five(lc, lm, lo, hi, hist):
        """rows of the frame forced through each line of step C: (1) the history's ids changed in a band: no history; (2) the lo ids changed
        in a band: no sample counts; both bands cross: the unguided mean; where the lo colours there are NaN as well: nothing"""
        Hp, Wp = hist.shape[1:3]
        hist.view(I32)[1, :, : max(1, Wp // 2), 3] += 9
        lo["id"][: max(1, LH // 2), :] += 5
        lc[: max(1, LH // 4), : max(1, LW // 4)] = np.nan
    add("five_branches", base, (0.0, 0.0), edit=five, radius=r1)
    return out


_refs = {}


def reference_results(shape):
    """[(name, kw, results with the branch plane)] of cases(shape) by the numpy reference, computed once per process"""
    if shape not in _refs:
        _refs[shape] = [(name, kw, temporal_upsample(branches=True, **kw)) for name, kw in cases(shape)]
    return _refs[shape]
