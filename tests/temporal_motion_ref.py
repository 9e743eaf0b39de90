"""Reference of art_temporal_motion_device written from the header comment of include/art_hip.h: art_temporal_device's steps
(tests/temporal_ref.py holds them for the call without motion) with the three changes of step 3 that the motion plane brings, in plain
numpy.  With motion None it IS temporal_ref.temporal.  Also the call through the g++ build of the product's text (tests/motion_host)
and the synthetic motion cases the CPU and GPU tests share."""
import ctypes as C

import numpy as np

import motion_ref as M
import temporal_ref as T
from temporal_ref import F, I32, _dot, _finite3, _rows, camera


def temporal(color, moments, n_colours, cam_cur, cam_prev=None, hist=None, normal=None, depth=None, ids=None, max_history=64, depth_tol=0.05,
             normal_min=0.9, scale=1.0, motion=None):
    """temporal_ref.temporal's arguments and results, plus motion [H, W, 3] float32 or None"""
    if motion is None:
        return T.temporal(color, moments, n_colours, cam_cur, cam_prev, hist, normal, depth, ids, max_history, depth_tol, normal_min, scale)
    with np.errstate(all="ignore"):
        color = np.asarray(color, F)
        H, W = color.shape[:2]
        moments = np.asarray(moments, F).reshape(H, W, 2)
        motion = np.asarray(motion, F).reshape(H, W, 3)
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
            if depth is None:                                        # no reprojection, and the motion is not read
                fx, fy, e = X + F(0.5), Y + F(0.5), z
            else:                                                    # equal cameras no longer switch it off
                rx, ry = (X + F(0.5)) - F(W) / F(2), (Y + F(0.5)) - F(H) / F(2)
                rz = np.full((H, W), cur["cam_z"], F)
                li = F(1) / np.sqrt(_dot(rx, ry, rz, rx, ry, rz))
                t = _rows(cur["M"], li * rx, li * ry, li * rz)
                lj = F(1) / np.sqrt(_dot(*t, *t))
                d = [lj * t[k] for k in range(3)]
                ok &= np.isfinite(motion).all(-1)                    # a delta that is not finite: NO HISTORY
                v = [((cur["pos"][k] + z * d[k]) + motion[..., k]) - prev["pos"][k] for k in range(3)]
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


def temporal_host(color, moments, n_colours, cam_cur, cam_prev=None, hist=None, normal=None, depth=None, ids=None, max_history=64, depth_tol=0.05,
                  normal_min=0.9, scale=1.0, motion=None):
    """the same call through csrc/art_temporal.h compiled by g++ (tests/motion_host): (hist_out, out, variance, length)"""
    color = np.ascontiguousarray(color, F)
    H, W = color.shape[:2]
    arrs = [color, np.ascontiguousarray(moments, F)] + [None if x is None else np.ascontiguousarray(x, F) for x in (normal, depth)]
    arrs.append(None if ids is None else np.ascontiguousarray(ids, I32))
    arrs.append(None if motion is None else np.ascontiguousarray(motion, F))
    arrs.append(None if hist is None else np.ascontiguousarray(hist, F))
    p = T.Params()
    p.cur = T.c_camera(cam_cur, W, H)
    if hist is not None:
        p.prev = T.c_camera(cam_prev, hist.shape[2], hist.shape[1])
    p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = n_colours, max_history, scale, depth_tol, normal_min
    new = np.zeros((3, H, W, 4), F)
    outs = [np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), F)]
    rc = M.host_lib().mh_temporal_motion(C.addressof(p), *[None if x is None else x.ctypes.data for x in arrs], new.ctypes.data, *[x.ctypes.data for x in outs])
    if rc:
        raise RuntimeError("mh_temporal_motion refused its arguments (%d)" % rc)
    return (new,) + tuple(outs)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
def pixel_shift(camr, fr, sx, sy):
    """the motion plane that takes every hit pixel of frame fr (temporal_ref.frame under camera camr, which looks along -z) back by
    (sx, sy) pixels in the previous frame of the same camera: a world displacement parallel to the image plane, scaled by the depth"""
    H, W = fr["depth"].shape
    c = camera(camr, W, H)
    # a point at distance z along the ray through pixel (x, y) lies at camera-space (rx, ry, cam_z) * z / |r|: one pixel is z / |r| wide
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5 - W / 2.0, np.arange(H, dtype=np.float64) + 0.5 - H / 2.0)
    r = np.sqrt(X * X + Y * Y + float(c["cam_z"]) ** 2)
    s = fr["depth"].astype(np.float64) / r
    d_cam = np.stack([sx * s, sy * s, np.zeros_like(s)], -1)
    return (d_cam @ c["M"].astype(np.float64).T).astype(F)


def cases(W, H):
    """(name, keyword arguments of temporal()) at one frame size: zero motion, constant shifts of whole and fractional pixels, motion out
    of the frame, motion that is not finite, equal cameras with motion, and the optional planes"""
    nc = 2
    base = T.cam()
    kw0 = dict(n_colours=nc, scale=1.0 / nc, max_history=16, depth_tol=0.05, normal_min=0.9)
    h = T.first_history(W, H, base, nc)
    out = []

    def add(name, cur_cam, shift=(0.0, 0.0), prev_cam=base, edit=None, drop=(), seed=1):
        fr = T.frame(cur_cam, W, H, seed=seed, n_colours=nc)
        mo = pixel_shift(cur_cam, fr, *shift)
        if edit:
            mo = edit(mo)
        for k in drop:
            fr[k] = None
        out.append((name, dict(kw0, cam_cur=cur_cam, cam_prev=prev_cam, hist=h.copy(), motion=mo, **fr)))

    moving = T.cam((0.05, 0.01, 0.0), yaw=0.004)
    add("zero_equal_cameras", base)
    add("zero_moving_camera", moving)
    add("whole_pixels_equal_cameras", base, (2.0, -1.0))
    add("fractional_pixels_equal_cameras", base, (0.37, 1.62))
    add("fractional_pixels_moving_camera", moving, (-1.25, 0.5))
    add("out_of_the_frame", base, (W + 3.0, 0.0))
    add("half_out_of_the_frame", base, (W / 2.0 + 0.25, H / 2.0))

    def bad(mo):
        mo = mo.copy()
        flat = mo.reshape(-1, 3)
        n = flat.shape[0]
        flat[0 % n, 0] = np.nan; flat[(n // 3) % n, 1] = np.inf; flat[(2 * n // 3) % n, 2] = -np.inf; flat[n - 1] = np.nan
        return mo
    add("not_finite_equal_cameras", base, (0.5, 0.0), edit=bad)
    add("not_finite_moving_camera", moving, edit=bad)
    add("huge", base, edit=lambda mo: (mo + F(3e38)).astype(F))
    for k in ("normal", "depth", "ids"):
        add("no_" + k, base, (1.5, 0.25), drop=(k,))
    out.append(("first_frame", dict(out[2][1], hist=None, cam_prev=None)))
    return out
