"""The product's motion text compiled by g++ (tests/motion_host: csrc/art_motion.h and the motion path of csrc/art_temporal.h) against the
numpy references written from the header (tests/motion_ref.py, tests/temporal_motion_ref.py), bit for bit, on synthetic hits and
frames.  No GPU."""
import numpy as np
import pytest

import motion_ref as M
import temporal_motion_ref as TM
import temporal_ref as T

F = np.float32


def signbits(a):
    return np.signbit(np.asarray(a, F))


# ---- the motion plane -------------------------------------------------------------------------------------------------------------
def synthetic_hits(K, n, ntris, seed, ninst=0, shift=0):
    """K * n rays: every class and misses at random, (u, v) with edges and corners among them"""
    rng = np.random.default_rng(seed)
    N = K * n
    cls = rng.choice([M.MISS, M.SPHERE, M.CORNELL, M.QUAD, M.BFTRI, M.TRI, M.TRI, M.TRI], N)
    tri = rng.integers(0, ntris, N)
    index = np.where(cls == M.TRI, tri if not ninst else (rng.integers(0, ninst, N) << shift) | tri, rng.integers(0, 3, N))
    u, v = rng.uniform(0, 1, N), rng.uniform(0, 1, N)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    special = [(0, 0), (1, 0), (0, 1), (0.5, 0.5), (0, 0.3), (0.7, 0), (0.25, 0.75), (1e-8, 1e-8), (-1e-7, 0.5), (0.5, -1e-7), (0.6, 0.6)]
    for k, (a, b) in enumerate(special):
        u[k::37] = a; v[k::37] = b
    t = rng.uniform(0.5, 30.0, N)
    d = rng.normal(size=(N, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return cls, index, t.astype(F), u.astype(F), v.astype(F), d.astype(F)


def flat_mesh(nverts, ntris, seed):
    rng = np.random.default_rng(seed)
    cur = rng.uniform(-3, 3, (nverts, 3)).astype(F)
    idx = rng.integers(0, nverts, (ntris, 3)).astype(np.int32)
    return idx, cur


@pytest.mark.parametrize("K", [1, 4])
def test_flat_plane_every_class_edges_and_corners(K):
    n, nverts, ntris = 301, 90, 130
    idx, cur = flat_mesh(nverts, ntris, 5)
    rng = np.random.default_rng(6)
    prev = (cur + rng.normal(0, 0.2, cur.shape)).astype(F)
    still = np.unique(idx[:40])                     # the first 40 triangles do not move
    prev[still] = cur[still]
    cls, index, t, u, v, d = synthetic_hits(K, n, ntris, 7)
    cam = np.array([0.3, -0.2, 4.0], F)
    per_ray = M.deltas(cls, index, t, u, v, d, cam, idx=idx, cur=cur, prev=prev)
    ref = M.plane(per_ray.reshape(K, n, 3))
    got = M.plane_host(K, cls, index, t, u, v, d, cam, idx=idx, cur=cur, prev=prev)
    assert M.differ(got, ref) == 0
    # what is not a CLOSEST triangle, and every unmoved triple, gives exactly +0
    zero = (cls != M.TRI) | (index < 40)
    assert (per_ray[zero] == 0).all() and not signbits(per_ray[zero]).any()
    assert (per_ray[(cls == M.TRI) & (index >= 40)] != 0).any()
    for c in (M.MISS, M.SPHERE, M.CORNELL, M.QUAD, M.BFTRI, M.TRI):
        assert (cls == c).any()
    # no vertex arrays, or prev equal to cur: all +0
    for kw in (dict(), dict(idx=idx, cur=cur, prev=cur.copy())):
        got = M.plane_host(K, cls, index, t, u, v, d, cam, **kw)
        assert (got == 0).all() and not signbits(got).any()
        assert M.differ(got, M.plane(M.deltas(cls, index, t, u, v, d, cam, **kw).reshape(K, n, 3))) == 0


def test_flat_plane_vertices_that_are_not_finite():
    K, n, nverts, ntris = 4, 120, 50, 60
    idx, cur = flat_mesh(nverts, ntris, 15)
    prev = (cur + F(0.1)).astype(F)
    prev[3, 0] = np.nan; prev[7, 1] = np.inf; cur[11, 2] = -np.inf; cur[13] = np.inf; prev[13] = np.inf
    cls, index, t, u, v, d = synthetic_hits(K, n, ntris, 17)
    cam = np.zeros(3, F)
    ref = M.plane(M.deltas(cls, index, t, u, v, d, cam, idx=idx, cur=cur, prev=prev).reshape(K, n, 3))
    got = M.plane_host(K, cls, index, t, u, v, d, cam, idx=idx, cur=cur, prev=prev)
    assert M.differ(got, ref) == 0 and not np.isfinite(ref).all() and np.isfinite(ref).any()       # stored as they are


def rigid(rng, n, scale=False):
    """n object -> world 3 x 4 matrices and their inverses (binary64 inverse rounded once: any inverse will do for the comparison)"""
    m, mi = np.zeros((n, 12), F), np.zeros((n, 12), F)
    for j in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a = q * (rng.uniform(0.5, 2.0, 3) if scale else 1.0)
        tr = rng.uniform(-4, 4, 3)
        m4 = np.eye(4); m4[:3, :3] = a; m4[:3, 3] = tr
        m[j] = m4[:3].reshape(12); mi[j] = np.linalg.inv(m4)[:3].reshape(12)
    return m, mi


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("ninst,shift", [(1, 7), (3, 7), (70, 9)])
def test_instanced_plane(K, ninst, shift):
    n, ntris = 257, 100
    rng = np.random.default_rng(100 + ninst)
    m_cur, minv = rigid(rng, ninst, scale=True)
    prev = m_cur.copy()                              # instance j: j % 4 == 0 equal, 1 translated, 2 rotated, 3 scaled
    other, _ = rigid(rng, ninst)
    for j in range(ninst):
        if j % 4 == 1 or ninst == 1:
            prev[j, 3::4] += np.array([0.3, -0.1, 0.2], F)
        elif j % 4 == 2:
            prev[j] = other[j]
        elif j % 4 == 3:
            prev[j].reshape(3, 4)[:, :3] *= F(1.1)
    if ninst > 1:
        prev[0] = m_cur[0]
    cls, index, t, u, v, d = synthetic_hits(K, n, ntris, 21, ninst, shift)
    cam = np.array([0.0, 2.5, 12.0], F)
    kw = dict(m_cur=m_cur, minv_cur=minv, prev_m=prev, inst_shift=shift)
    per_ray = M.deltas(cls, index, t, u, v, d, cam, **kw)
    got = M.plane_host(K, cls, index, t, u, v, d, cam, **kw)
    assert M.differ(got, M.plane(per_ray.reshape(K, n, 3))) == 0
    equal = (cls != M.TRI) | ((index >> shift) % 4 == 0) if ninst > 1 else (cls != M.TRI)
    assert (per_ray[equal] == 0).all() and (per_ray[~equal] != 0).any()
    # no previous matrices: zero
    kw0 = dict(kw, prev_m=None)
    got = M.plane_host(K, cls, index, t, u, v, d, cam, **kw0)
    assert (got == 0).all() and not signbits(got).any()
    # matrices that are not finite
    bad = prev.copy(); bad[0, 0] = np.nan; bad[-1, 7] = np.inf
    kwb = dict(kw, prev_m=bad)
    ref = M.plane(M.deltas(cls, index, t, u, v, d, cam, **kwb).reshape(K, n, 3))
    assert M.differ(M.plane_host(K, cls, index, t, u, v, d, cam, **kwb), ref) == 0 and not np.isfinite(ref).all()


# ---- the temporal call with motion ------------------------------------------------------------------------------------------------
def same(a, b):
    return all(T.differ(x, y) == 0 for x, y in zip(a, b))


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: "%dx%d" % s)
def test_temporal_motion_host_equals_the_reference(size):
    W, H = size
    for name, kw in TM.cases(W, H):
        assert same(TM.temporal_host(**kw), TM.temporal(**kw)), name


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: "%dx%d" % s)
def test_without_motion_it_is_the_existing_call(size):
    W, H = size
    for name, kw in T.cases(W, H):
        ref = T.temporal(**kw)
        assert same(TM.temporal_host(**kw), ref) and same(T.temporal_host(**kw), ref), name


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: "%dx%d" % s)
def test_zero_motion_equals_the_existing_path(size):
    """between different cameras zero motion gives the existing call's bits; between equal cameras the old rule skips the projection, so
    the two agree except for fractional parts of exactly 0: the history lengths agree to rounding and the guides are the same words"""
    W, H = size
    for name, kw in T.cases(W, H):
        if kw["hist"] is None:
            continue
        zero = np.zeros((H, W, 3), F)
        ref, got = T.temporal(**kw), TM.temporal(**kw, motion=zero)
        cur, prev = T.camera(kw["cam_cur"], W, H), T.camera(kw["cam_prev"], kw["hist"].shape[2], kw["hist"].shape[1])
        if kw["depth"] is None or cur["words"] != prev["words"]:
            assert same(got, ref), name
        else:
            assert T.differ(got[0][2], ref[0][2]) == 0 and T.differ(got[0][1][..., 2:], ref[0][1][..., 2:]) == 0, name      # the frame's guides
            # The projection puts the pixel back on itself within a few ulp of its coordinate (|coordinate| <= 65 here: under 1e-4 of a
            # pixel), so the pixel's own record weighs 1 - O(1e-4) and its neighbours O(1e-4).  Where the existing path found a history,
            # this one finds the same within that share of the neighbours' values (colours within a factor of ten of each other: 1e-3);
            # where the pixel's own record is refused a neighbour's may now be taken, and nothing is claimed.
            has = (ref[3] > kw["n_colours"]) & np.isfinite(ref[1]).all(-1) & np.isfinite(got[1]).all(-1)
            assert has.any() or W * H < 8, name
            with np.errstate(invalid="ignore"):                   # (colours that are not finite on both sides are outside `has`)
                assert (np.abs(got[3] - ref[3])[has] <= 1e-3 * ref[3][has]).all(), name
                assert (np.abs(got[1] - ref[1])[has] <= 1e-3 * (1 + np.abs(ref[1][has]))).all(), name


def test_equal_cameras_with_motion_find_the_shifted_history():
    """cameras at rest, the whole picture moved by exactly two pixels: the history of pixel (x, y) is found at (x + 2, y)"""
    W, H = 64, 33
    base = T.cam()
    fr = T.frame(base, W, H, seed=1)
    flat = dict(fr, depth=np.where(fr["depth"] > 0, F(10.0), F(0.0)), ids=np.where(fr["depth"] > 0, 1, -1).astype(np.int32),
                normal=np.where((fr["depth"] > 0)[..., None], np.array([0, 0, 1], F), F(0)).astype(F))
    kw = dict(n_colours=2, scale=0.5, max_history=16, depth_tol=0.5, normal_min=0.9)
    h = T.temporal(cam_cur=base, **flat, **kw)[0]
    mo = TM.pixel_shift(base, flat, 2.0, 0.0)
    still = T.temporal(cam_cur=base, cam_prev=base, hist=h, **flat, **kw)
    moved = TM.temporal(cam_cur=base, cam_prev=base, hist=h, motion=mo, **flat, **kw)
    assert (still[3] == 4).all()
    inside = np.zeros((H, W), bool); inside[:, :W - 3] = True
    assert (np.abs(moved[3][inside] - 4) < 1e-3).all() and (moved[3][:, W - 1] == 2).all()
    want = F(0.5) * (F(0.5) * flat["color"][:, :W - 3]) + F(0.5) * (F(0.5) * flat["color"][:, 2:W - 1])
    assert np.abs(moved[1][:, :W - 3] - want).max() < 1e-2
