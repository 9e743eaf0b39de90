"""Reference of the motion plane of art_render_aovs_motion_device written from the header comment of include/art_hip.h alone: plain numpy
over the rays, binary32 arrays, every operation in the order the header writes it.  Also the loader of tests/motion_host/
libmotion_host.so -- the product's per-hit text (csrc/art_motion.h) and the motion path of csrc/art_temporal.h compiled by g++."""
import ctypes as C
import os
import subprocess

import numpy as np

F = np.float32
I32 = np.int32
HERE = os.path.dirname(os.path.abspath(__file__))
# hit classes (the key's top bits, csrc/art_scene.h); MISS is this file's own
MISS, SPHERE, CORNELL, QUAD, BFTRI, TRI = -1, 0, 1, 2, 3, 4


def T(m, k, px, py, pz):
    """row k of 3 x 4 matrices m[..., 12] applied to points"""
    return ((m[..., 4 * k] * px + m[..., 4 * k + 1] * py) + m[..., 4 * k + 2] * pz) + m[..., 4 * k + 3]


def deltas(cls, index, t, u, v, dirs=None, cam_pos=None, idx=None, cur=None, prev=None, m_cur=None, minv_cur=None, prev_m=None, inst_shift=0):
    """per ray: cls [n] (the constants above), index [n] (the key's index), t, u, v [n] float32, dirs [n, 3] -> delta [n, 3] float32.
    Flat scene: idx [ntris, 3], cur / prev [nverts, 3] (both or neither).  Instanced (m_cur is not None): m_cur, minv_cur [ninst, 12] the
    matrices in force, prev_m [ninst, 12] or None."""
    with np.errstate(all="ignore"):
        cls, index = np.asarray(cls), np.asarray(index).astype(np.int64)
        t, u, v = np.asarray(t, F), np.asarray(u, F), np.asarray(v, F)
        out = np.zeros((cls.shape[0], 3), F)
        tri = cls == TRI
        if not tri.any():
            return out
        if m_cur is not None:
            if prev_m is None:
                return out
            j = index[tri] >> inst_shift
            d = np.asarray(dirs, F)[tri]
            cam = np.asarray(cam_pos, F)
            pw = [cam[k] + t[tri] * d[:, k] for k in range(3)]
            mc, mi, mp = np.asarray(m_cur, F)[j], np.asarray(minv_cur, F)[j], np.asarray(prev_m, F).reshape(-1, 12)[j]
            po = [T(mi, k, *pw) for k in range(3)]
            out[tri] = np.stack([T(mp, k, *po) - T(mc, k, *po) for k in range(3)], -1)
            assert out.dtype == F
            return out
        if cur is None:
            return out
        tr = np.asarray(idx).reshape(-1, 3)[index[tri]]
        cur, prev = np.asarray(cur, F).reshape(-1, 3), np.asarray(prev, F).reshape(-1, 3)
        uu, vv = u[tri][:, None], v[tri][:, None]
        w = (F(1.0) - uu) - vv
        da, db, dc = (prev[tr[:, k]] - cur[tr[:, k]] for k in range(3))
        out[tri] = (w * da + vv * db) + uu * dc
        assert out.dtype == F
        return out


def plane(d):
    """d [K, n, 3] per-ray deltas -> [n, 3]: the AOV association"""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        return d[0] if d.shape[0] == 1 else ((((d[0] + d[1]) + d[2]) + d[3]) * F(0.25)).astype(F)


def from_hits(raw, dirs, cam_pos, **src):
    """raw [K, n, 11]: ArtHit words of a scene WITHOUT a REFERENCE_BF mesh (prim_type 2 is then a CLOSEST triangle); dirs [K, n, 3] -> the
    plane [n, 3]"""
    K = raw.shape[0]
    f = raw.view(F)
    out = []
    for s in range(K):
        hit = raw[s, :, 1] == 1
        cls = np.where(hit & (raw[s, :, 2] == 2), TRI, np.where(hit, CORNELL, MISS))
        out.append(deltas(cls, np.where(hit, raw[s, :, 3], 0), f[s, :, 0], f[s, :, 9], f[s, :, 10], dirs[s], cam_pos, **src))
    return plane(np.stack(out))


def words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def differ(a, b):
    """number of words that differ (NaNs of any payload count as equal to each other)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(((words(a) != words(b)) & ~(np.isnan(a) & np.isnan(b))).sum())


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
_host = None


def host_lib():
    global _host
    if _host is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "motion_host"), "libmotion_host.so"])
        L = C.CDLL(os.path.join(HERE, "motion_host", "libmotion_host.so"))
        L.mh_plane.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 11 + [C.c_int32, C.c_void_p]
        L.mh_plane.restype = C.c_int
        L.mh_temporal_motion.argtypes = [C.c_void_p] * 12
        L.mh_temporal_motion.restype = C.c_int
        _host = L
    return _host


KEY_MISS = 0x7FFFFFFF


def keys(cls, index):
    cls, index = np.asarray(cls).astype(np.int64), np.asarray(index).astype(np.int64)
    return np.where(cls == MISS, KEY_MISS, (np.maximum(cls, 0) << 28) | index).astype(np.uint32)


def plane_host(K, cls, index, t, u, v, dirs, cam_pos, idx=None, cur=None, prev=None, m_cur=None, minv_cur=None, prev_m=None, inst_shift=0):
    """the plane of n pixels with K rays each (ray s of pixel l at s * n + l) through csrc/art_motion.h compiled by g++"""
    n = len(cls) // K
    key = keys(cls, index)
    arr = lambda x, dt=F: None if x is None else np.ascontiguousarray(x, dt)
    t, u, v, dirs, cam = arr(t), arr(u), arr(v), arr(dirs), arr(cam_pos)
    idx, cur, prev, prev_m = arr(idx, I32), arr(cur), arr(prev), arr(prev_m)
    inst = None
    if m_cur is not None:                       # DevInstance records: 32 words, m then minv
        inst = np.zeros((len(m_cur), 32), F)
        inst[:, :12] = m_cur; inst[:, 12:24] = minv_cur
    out = np.full((n, 3), -7.0, F)
    p = lambda x: None if x is None else x.ctypes.data
    rc = host_lib().mh_plane(K, n, p(key), p(t), p(u), p(v), p(dirs), p(cam), p(idx), p(cur), p(prev), p(inst), p(prev_m), inst_shift, p(out))
    assert rc == 0
    return out
