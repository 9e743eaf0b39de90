"""Reference of art_temporal_device written from the header comment of include/art_hip.h alone: plain numpy over the pixels, binary32
arrays except where the header names binary64, a Python loop over the four taps.  Also the loader of tests/temporal_host/
libtemporal_host.so -- the product's per-pixel text (csrc/art_temporal.h) compiled by g++ -- and the synthetic frames and cases the
temporal tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

from denoise_ref import F, _finite3, differ      # noqa: F401 (differ: for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
I32 = np.int32


def camera(cam, width, height):
    """(cam_pos, cam_matrix), the frame's size -> dict with the binary32 3 x 3, its inverse and cam_z; None where the header refuses it"""
    pos = np.asarray(cam[0], F).reshape(3)
    m = np.asarray(cam[1], F).reshape(16)
    if not (np.isfinite(pos).all() and np.isfinite(m).all()) or m[3] != 0 or m[7] != 0 or m[11] != 0:
        return None
    M = m.reshape(4, 4)[:3, :3].copy()
    a = [[float(M[r, k]) for k in range(3)] for r in range(3)]           # Python floats: every operation rounds to binary64
    c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1]
    c01 = a[1][0] * a[2][2] - a[1][2] * a[2][0]
    c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0]
    det = (a[0][0] * c00 - a[0][1] * c01) + a[0][2] * c02
    if det == 0.0 or not np.isfinite(det):
        return None
    inv = [c00, a[0][2] * a[2][1] - a[0][1] * a[2][2], a[0][1] * a[1][2] - a[0][2] * a[1][1],
           a[1][2] * a[2][0] - a[1][0] * a[2][2], a[0][0] * a[2][2] - a[0][2] * a[2][0], a[0][2] * a[1][0] - a[0][0] * a[1][2],
           c02, a[0][1] * a[2][0] - a[0][0] * a[2][1], a[0][0] * a[1][1] - a[0][1] * a[1][0]]
    with np.errstate(all="ignore"):
        inv = np.array([v / det for v in inv], np.float64).astype(F).reshape(3, 3)
    if not np.isfinite(inv).all():
        return None
    return dict(pos=pos, M=M, I=inv, cam_z=-F(width) / F(1.0), W=int(width), H=int(height), words=(pos.tobytes(), m.tobytes(), int(width), int(height)))


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _rows(M, x, y, z):
    return [(M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z for k in range(3)]


def temporal(color, moments, n_colours, cam_cur, cam_prev=None, hist=None, normal=None, depth=None, ids=None, max_history=64, depth_tol=0.05,
             normal_min=0.9, scale=1.0):
    """color [H, W, 3], moments [H, W, 2], normal [H, W, 3], depth [H, W] float32, ids [H, W] int32, hist [3, Hp, Wp, 4] float32 or None
    -> (hist_out [3, H, W, 4], out [H, W, 3], variance [H, W], length [H, W]) float32"""
    with np.errstate(all="ignore"):
        color = np.asarray(color, F)
        H, W = color.shape[:2]
        moments = np.asarray(moments, F).reshape(H, W, 2)
        cur = camera(cam_cur, W, H)
        assert cur is not None
        scale, depth_tol, normal_min, n_cur = F(scale), F(depth_tol), F(normal_min), F(n_colours)
        c = scale * color
        m1, m2 = moments[..., 0] / n_cur, moments[..., 1] / n_cur
        z = np.asarray(depth, F) if depth is not None else np.zeros((H, W), F)
        pid = np.asarray(ids, I32) if ids is not None else np.zeros((H, W), I32)
        N = np.asarray(normal, F) if normal is not None else np.zeros((H, W, 3), F)
        own = np.full((H, W), hist is None)
        if depth is not None:
            own |= ~((z > 0) & np.isfinite(z))
        if normal is not None:
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
            if depth is None or cur["words"] == prev["words"]:
                fx, fy, e = X + F(0.5), Y + F(0.5), z
            else:
                rx, ry = (X + F(0.5)) - F(W) / F(2), (Y + F(0.5)) - F(H) / F(2)
                rz = np.full((H, W), cur["cam_z"], F)
                li = F(1) / np.sqrt(_dot(rx, ry, rz, rx, ry, rz))
                t = _rows(cur["M"], li * rx, li * ry, li * rz)
                lj = F(1) / np.sqrt(_dot(*t, *t))
                d = [lj * t[k] for k in range(3)]
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
                if depth is not None:
                    cnt &= np.abs(b[..., 2] - e) <= depth_tol * e
                if normal is not None:
                    cnt &= _dot(N[..., 0], N[..., 1], N[..., 2], g[..., 0], g[..., 1], g[..., 2]) >= normal_min
                if ids is not None:
                    cnt &= np.ascontiguousarray(b[..., 3]).view(I32) == pid
                fields = (a[..., 0], a[..., 1], a[..., 2], a[..., 3], b[..., 0], b[..., 1])
                assert w.dtype == F
                sums = [np.where(cnt, s + w * f, s).astype(F) for s, f in zip(sums, fields)]
                wsum = np.where(cnt, wsum + w, wsum).astype(F)
        has = wsum > 0
        one = np.where(has, wsum, F(1))
        hr, hg, hb, hn, hm1, hm2 = [s / one for s in sums]
        cap = F(max_history) - n_cur
        f = np.where(hn > cap, cap / np.where(has, hn, F(1)), F(1)).astype(F)
        n = n_cur + f * hn
        a = n_cur / n
        b = F(1) - a
        blend = lambda x, h: np.where(has, a * x + b * h, x).astype(F)
        n = np.where(has, n, n_cur).astype(F)
        col = np.stack([blend(c[..., 0], hr), blend(c[..., 1], hg), blend(c[..., 2], hb)], axis=-1)
        m1, m2 = blend(m1, hm1), blend(m2, hm2)
        out = np.zeros((3, H, W, 4), F)
        out[0, ..., :3] = col; out[0, ..., 3] = n
        out[1, ..., 0] = m1; out[1, ..., 1] = m2; out[1, ..., 2] = z
        out.view(I32)[1, ..., 3] = pid
        out[2, ..., :3] = N
        n64, d1 = n.astype(np.float64), m1.astype(np.float64)
        D = m2.astype(np.float64) - d1 * d1
        D0 = np.where(D < 0.0, 0.0, D)
        var = np.where(n < 2, F(np.inf), ((D0 * (n64 / (n64 - 1.0))) / n64).astype(F)).astype(F)
        return out, col, var, n


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
class Camera(C.Structure):          # include/art_hip.h ArtTemporalCamera (its own mirror: the host library needs no package)
    _fields_ = [("cam_pos", C.c_float * 3), ("cam_matrix", C.c_float * 16), ("width", C.c_int32), ("height", C.c_int32)]


class Params(C.Structure):          # ArtTemporalParams
    _fields_ = [("cur", Camera), ("prev", Camera), ("n_colours", C.c_int32), ("max_history", C.c_int32), ("scale", C.c_float),
                ("depth_tol", C.c_float), ("normal_min", C.c_float)]


_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "temporal_host"), "libtemporal_host.so"])
        L = C.CDLL(os.path.join(HERE, "temporal_host", "libtemporal_host.so"))
        L.th_temporal.argtypes = [C.POINTER(Params)] + [C.c_void_p] * 10
        L.th_temporal.restype = C.c_int
        L.th_denoise_svgf_var.argtypes = [C.c_void_p] * 8
        L.th_denoise_svgf_var.restype = C.c_int
        _host = L
    return _host


def c_camera(cam, width, height, cls=Camera):
    pos = [float(v) for v in np.asarray(cam[0], F).reshape(3)]
    m = [float(v) for v in np.asarray(cam[1], F).reshape(16)]
    return cls((C.c_float * 3)(*pos), (C.c_float * 16)(*m), width, height)


def temporal_host(color, moments, n_colours, cam_cur, cam_prev=None, hist=None, normal=None, depth=None, ids=None, max_history=64, depth_tol=0.05,
                  normal_min=0.9, scale=1.0, want=(True, True, True)):
    """the same call through csrc/art_temporal.h compiled by g++; want: which of (out, variance, length) are asked for"""
    color = np.ascontiguousarray(color, F)
    H, W = color.shape[:2]
    arrs = [color, np.ascontiguousarray(moments, F)] + [None if x is None else np.ascontiguousarray(x, F) for x in (normal, depth)]
    arrs.append(None if ids is None else np.ascontiguousarray(ids, I32))
    arrs.append(None if hist is None else np.ascontiguousarray(hist, F))
    p = Params()
    p.cur = c_camera(cam_cur, W, H)
    if hist is not None:
        p.prev = c_camera(cam_prev, hist.shape[2], hist.shape[1])
    p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = n_colours, max_history, scale, depth_tol, normal_min
    new = np.zeros((3, H, W, 4), F)
    outs = [np.zeros((H, W, 3), F) if want[0] else None, np.zeros((H, W), F) if want[1] else None, np.zeros((H, W), F) if want[2] else None]
    rc = host_lib().th_temporal(C.byref(p), *[None if x is None else x.ctypes.data for x in arrs], new.ctypes.data,
                                *[None if x is None else x.ctypes.data for x in outs])
    if rc:
        raise RuntimeError("th_temporal refused its arguments (%d)" % rc)
    return (new,) + tuple(outs)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (7, 1), (13, 9), (64, 33), (130, 3)]          # (W, H)
IDENT = np.eye(4, dtype=F)


def cam(pos=(0.0, 0.0, 0.0), yaw=0.0):
    """a camera at pos, turned by yaw about y (it looks along -z at yaw 0)"""
    m = np.eye(4)
    m[0, 0] = m[2, 2] = np.cos(yaw); m[0, 2] = np.sin(yaw); m[2, 0] = -np.sin(yaw)
    return np.array(pos, F), m.astype(F)


def frame(camr, W, H, seed=0, n_colours=2):
    """the planes of a synthetic frame under camera camr: a wall at z = -10 (id 1) and, in front of it, a panel at z = -6 over 0.5 < x < 3
    (id 2, normal tilted), so that a moving camera uncovers wall behind the panel's edges; rays that look away from both miss (depth 0,
    normal 0, id -1).  Colour follows the world point plus noise; the moments belong to the colour read as the sum of n colours."""
    rng = np.random.default_rng(1000 * W + H + 17 * seed)
    c = camera(camr, W, H)
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5 - W / 2.0, np.arange(H, dtype=np.float64) + 0.5 - H / 2.0)
    r = np.stack([X, Y, np.full_like(X, float(c["cam_z"]))], -1)
    d = r @ c["M"].astype(np.float64).T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = c["pos"].astype(np.float64)
    with np.errstate(all="ignore"):
        t_wall = (-10.0 - o[2]) / d[..., 2]
        t_pan = (-6.0 - o[2]) / d[..., 2]
        xp = o[0] + t_pan * d[..., 0]
        pan = (t_pan > 0) & (xp > 0.5) & (xp < 3.0)
        wall = (t_wall > 0) & ~pan
        t = np.where(pan, t_pan, np.where(wall, t_wall, 0.0))
    P = o + t[..., None] * d
    depth = t.astype(F)
    ids = np.where(pan, 2, np.where(wall, 1, -1)).astype(I32)
    normal = np.zeros((H, W, 3), F)
    normal[wall] = (0.0, 0.0, 1.0)
    normal[pan] = np.array([0.6, 0.0, 0.8], F)
    base = 1.0 + 0.5 * np.sin(P[..., 0:1] * 1.3 + np.arange(3)) + 0.3 * np.cos(P[..., 1:2] * 0.7)
    color = (n_colours * base * np.exp(rng.normal(0.0, 0.3, (H, W, 3)))).astype(F)
    lum = (0.2126 * color[..., 0] + 0.7152 * color[..., 1] + 0.0722 * color[..., 2]).astype(np.float64)
    rel = np.exp(rng.uniform(np.log(1e-2), np.log(2.0), (H, W)))
    mom = np.stack([lum, lum * lum / n_colours * (1.0 + rel * rel)], -1).astype(F)
    return dict(color=color, moments=mom, normal=normal, depth=depth, ids=ids)


def first_history(W, H, camr, n_colours=2, frames=1, **kw):
    """a history of the header's own making: `frames` frames at camera camr, from the reference"""
    h = None
    for k in range(frames):
        fr = frame(camr, W, H, seed=100 + k, n_colours=n_colours)
        h = temporal(n_colours=n_colours, cam_cur=camr, cam_prev=camr, hist=h, scale=1.0 / n_colours, **fr, **kw)[0]
    return h


def cases(W, H):
    """(name, keyword arguments of temporal()) at one frame size: the motions, the disocclusions, bad data and the optional planes"""
    nc = 2
    base = cam()
    kw0 = dict(n_colours=nc, scale=1.0 / nc, max_history=16, depth_tol=0.05, normal_min=0.9)
    h = first_history(W, H, base, nc)
    out = []

    def add(name, cur_cam, prev_cam=base, hist=h, seed=1, edit=None, drop=(), **over):
        fr = frame(cur_cam, W, H, seed=seed, n_colours=nc)
        hist = None if hist is None else hist.copy()
        if edit:
            edit(fr, hist)
        for k in drop:
            fr[k] = None
        out.append((name, dict(kw0, cam_cur=cur_cam, cam_prev=prev_cam, hist=hist, **fr, **over)))

    add("first_frame", base, hist=None)
    add("rest", base)
    add("rest_capped", base, hist=first_history(W, H, base, nc, frames=3, max_history=5), max_history=5)
    add("pan_subpixel", cam((0.013, 0.007, 0.0)))
    add("pan", cam((0.4, -0.1, 0.0)))
    add("rotate_y", cam(yaw=0.03))
    add("dolly_in", cam((0.0, 0.0, -1.5)))
    add("dolly_out", cam((0.0, 0.0, 2.0)))
    back = cam((2.0, 0.0, -8.0))                 # between the panel (behind it) and the wall (2 in front of it: most of the wall lands outside its frame)
    add("outside_and_behind", cam((0.0, 0.0, -4.0), yaw=-0.5), prev_cam=back, hist=first_history(W, H, back, nc))
    add("prev_other_size", cam((0.1, 0.0, 0.0)), hist=first_history(W + 3, H + 2, base, nc))

    def part(a):
        return (slice(0, max(1, a.shape[1] // 2)), slice(0, max(1, a.shape[2] * 2 // 3)))

    def e_depth(fr, hs): ys, xs = part(hs); hs[1, ys, xs, 2] += F(1.5)
    def e_normal(fr, hs): ys, xs = part(hs); hs[2, ys, xs, :3] *= F(-1)
    def e_id(fr, hs): ys, xs = part(hs); hs.view(I32)[1, ys, xs, 3] += 7
    def e_all(fr, hs): e_depth(fr, hs); e_normal(fr, hs); e_id(fr, hs)
    for name, e in (("depth_step", e_depth), ("normal_flip", e_normal), ("id_change", e_id), ("all_three", e_all)):
        add("disocclusion_" + name, cam((0.02, 0.0, 0.0)), edit=e)

    def spots(a, k):
        """k-th of a few pixel positions spread over the frame"""
        Hh, Ww = a.shape[:2]
        return ((k * 5 + 1) % Hh, (k * 7 + 2) % Ww)

    def e_bad_cur(fr, hs):
        fr["color"][spots(fr["color"], 0)] = np.nan; fr["color"][spots(fr["color"], 1)][1] = np.inf
        fr["moments"][spots(fr["color"], 2)][0] = np.nan
    def e_bad_hist(fr, hs):
        hs[0][spots(hs[0], 0)][0] = np.nan; hs[0][spots(hs[0], 1)][2] = -np.inf; hs[1][spots(hs[0], 2)][1] = np.nan
        hs[0][spots(hs[0], 3)][3] = 0.0; hs[0][spots(hs[0], 4)][3] = np.nan; hs[0][spots(hs[0], 5)][3] = -1.0
    def e_bad_guides(fr, hs):
        fr["depth"][spots(fr["depth"], 0)] = np.nan; fr["depth"][spots(fr["depth"], 1)] = np.inf; fr["depth"][spots(fr["depth"], 2)] = -1.0
        fr["normal"][spots(fr["depth"], 3)][1] = np.nan; fr["depth"][spots(fr["depth"], 4)] = 0.0
        hs[1][spots(hs[0], 5)][2] = np.nan; hs[2][spots(hs[0], 6)][0] = np.inf; hs[1][spots(hs[0], 7)][2] = 0.0
    for mv, c2 in (("rest", base), ("pan", cam((0.3, 0.0, 0.0)))):
        add("bad_cur_colour_" + mv, c2, edit=e_bad_cur)
        add("bad_history_" + mv, c2, edit=e_bad_hist)
        add("bad_guides_" + mv, c2, edit=e_bad_guides)
    add("misses", cam(yaw=1.2), prev_cam=cam(yaw=1.15), hist=first_history(W, H, cam(yaw=1.15), nc))
    for k in ("normal", "depth", "ids"):
        add("no_" + k, cam((0.05, 0.0, 0.0)), drop=(k,))
    add("no_guides", cam((0.05, 0.0, 0.0)), drop=("normal", "depth", "ids"))
    return out


def run_chain(fn, W, H, frames=5):
    """five frames along a pan, hist_out fed back as hist_in, through fn (temporal or a wrapper with its signature): the last results"""
    h, prev, res = None, None, None
    for k in range(frames):
        c = cam((0.05 * k, 0.01 * k, -0.1 * k), yaw=0.004 * k)
        fr = frame(c, W, H, seed=k, n_colours=2)
        res = fn(n_colours=2, cam_cur=c, cam_prev=prev, hist=h, scale=0.5, max_history=7, depth_tol=0.05, normal_min=0.9, **fr)
        h, prev = res[0], c
    return res
