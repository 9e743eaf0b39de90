"""art_temporal_device without a GPU: the product's per-pixel text (csrc/art_temporal.h) compiled by g++ against the numpy reference written
from the header comment (tests/temporal_ref.py), bit for bit, on the motions, disocclusions, bad data and optional planes the GPU test
runs; the properties the header promises; the refusals of the host build."""
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as T

F = np.float32


def same(a, b):
    return all(T.differ(x, y) == 0 for x, y in zip(a, b))


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_build_equals_the_numpy_reference(size):
    W, H = size
    for name, kw in T.cases(W, H):
        assert same(T.temporal_host(**kw), T.temporal(**kw)), name


def test_chain_of_five_frames():
    got, ref = T.run_chain(T.temporal_host, 64, 33), T.run_chain(T.temporal, 64, 33)
    assert same(got, ref) and (ref[3] > 2).any()


def test_optional_outputs():
    W, H = 13, 9
    kw = dict(T.cases(W, H))["pan"]
    full = T.temporal_host(**kw)
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = T.temporal_host(**kw, want=want)
        assert T.differ(got[0], full[0]) == 0
        for k in range(3):
            assert (got[1 + k] is None) == (not want[k]) and (got[1 + k] is None or T.differ(got[1 + k], full[1 + k]) == 0)


@pytest.mark.parametrize("fn", [T.temporal, T.temporal_host], ids=["numpy", "host_build"])
def test_cameras_at_rest_add_lengths_exactly_and_the_cap_engages(fn):
    """identical cameras: every pixel that hit something maps to itself with weight exactly 1, so the history is the previous record
    itself: length n_cur + n_prev until max_history, then max_history; colour is the length-weighted mean"""
    W, H = 13, 9
    c = T.cam()
    h, lengths = None, []
    for k in range(5):
        fr = T.frame(c, W, H, seed=k)
        h, out, var, n = fn(n_colours=2, cam_cur=c, cam_prev=c, hist=h, scale=0.5, max_history=7, **fr)
        hit = fr["depth"] > 0
        lengths.append(np.unique(n[hit]).tolist())
        assert (n[~hit] == 2).all() and np.isinf(var[n < 2]).all() and np.isfinite(var[n >= 2]).all()
    assert lengths == [[2.0], [4.0], [6.0], [7.0], [7.0]]
    # two frames, by hand: a = 2 / 4
    f0, f1 = T.frame(c, W, H, seed=0), T.frame(c, W, H, seed=1)
    h0 = fn(n_colours=2, cam_cur=c, scale=0.5, **f0)[0]
    out = fn(n_colours=2, cam_cur=c, cam_prev=c, hist=h0, scale=0.5, **f1)[1]
    hit = f1["depth"] > 0
    want = F(0.5) * (F(0.5) * f1["color"]) + F(0.5) * (F(0.5) * f0["color"])
    assert np.array_equal(out[hit], want[hit]) and np.array_equal(out[~hit], (F(0.5) * f1["color"])[~hit])


@pytest.mark.parametrize("fn", [T.temporal, T.temporal_host], ids=["numpy", "host_build"])
def test_disocclusion_restarts_the_history(fn):
    W, H = 64, 33
    cs = dict(T.cases(W, H))
    for name in ("depth_step", "normal_flip", "id_change", "all_three"):
        kw = cs["disocclusion_" + name]
        n = fn(**kw)[3]
        assert (n[: H // 2 - 1, : W * 2 // 3 - 1] == 2).all() and (n[H // 2 + 1:, :][kw["depth"][H // 2 + 1:, :] > 0] > 2).mean() > 0.9, name


@pytest.mark.parametrize("fn", [T.temporal, T.temporal_host], ids=["numpy", "host_build"])
def test_a_bad_colour_does_not_stay(fn):
    """a NaN in the current colour goes into the history as it is; the next frame does not count that record and starts again"""
    W, H = 13, 9
    c = T.cam()
    f0, f1 = T.frame(c, W, H, seed=0), T.frame(c, W, H, seed=1)
    f0["color"][4, 6] = np.nan
    h0 = fn(n_colours=2, cam_cur=c, scale=0.5, **f0)[0]
    assert np.isnan(h0[0, 4, 6, :3]).all()
    h1, out, var, n = fn(n_colours=2, cam_cur=c, cam_prev=c, hist=h0, scale=0.5, **f1)
    assert np.isfinite(out).all() and n[4, 6] == 2 and n[4, 5] == 4


def test_the_cases_hold_the_populations_they_are_named_for():
    """at the sizes with room for it: 'outside_and_behind' has pixels behind the previous camera, pixels in front of it that land outside
    its frame, and neither kind finds history; 'misses' has hit and miss pixels, and only hits find history"""
    for W, H in ((13, 9), (64, 33), (130, 3)):
        cs = dict(T.cases(W, H))
        kw = cs["outside_and_behind"]
        cur, prev = T.camera(kw["cam_cur"], W, H), T.camera(kw["cam_prev"], W, H)
        X, Y = np.meshgrid(np.arange(W) + 0.5 - W / 2.0, np.arange(H) + 0.5 - H / 2.0)
        d = np.stack([X, Y, np.full_like(X, float(cur["cam_z"]))], -1) @ cur["M"].astype(np.float64).T
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        v = cur["pos"].astype(np.float64) + kw["depth"][..., None].astype(np.float64) * d - prev["pos"].astype(np.float64)
        q = v @ prev["I"].astype(np.float64).T
        hit = kw["depth"] > 0
        front = hit & (q[..., 2] * float(prev["cam_z"]) > 0)
        with np.errstate(all="ignore"):
            fx, fy = q[..., 0] * float(prev["cam_z"]) / q[..., 2] + W / 2.0, q[..., 1] * float(prev["cam_z"]) / q[..., 2] + H / 2.0
        outside = front & ((fx < -0.5) | (fx > W + 0.5) | (fy < -0.5) | (fy > H + 0.5))
        assert (hit & ~front).any() and outside.any(), (W, H)
        n = T.temporal(**kw)[3]
        assert (n[(hit & ~front) | outside] == 2).all()
        kw = cs["misses"]
        hit, n = kw["depth"] > 0, T.temporal(**kw)[3]
        assert hit.any() and (~hit).any() and (n[~hit] == 2).all() and (n[hit] > 2).any(), (W, H)


def test_params_are_refused_by_the_host_build():
    c = T.cam()
    color, mom = np.ones((2, 2, 3), F), np.ones((2, 2, 2), F)
    h = T.temporal(color, mom, 2, c)[0]
    bad_t, bad_s = (np.zeros(3, F), np.eye(4, dtype=F)), (np.zeros(3, F), np.eye(4, dtype=F))
    bad_t[1][1, 3] = 1.0; bad_s[1][2, 2] = 0.0
    nan_pos = (np.array([0, np.nan, 0], F), np.eye(4, dtype=F))
    for kw in (dict(n_colours=0), dict(max_history=1), dict(max_history=(1 << 24) + 1), dict(scale=np.inf), dict(depth_tol=np.nan), dict(normal_min=np.nan),
               dict(cam_cur=bad_t), dict(cam_cur=bad_s), dict(cam_cur=nan_pos), dict(hist=h, cam_prev=bad_t), dict(hist=h, cam_prev=bad_s)):
        args = dict(n_colours=2, cam_cur=c, cam_prev=c)
        args.update(kw)
        with pytest.raises(RuntimeError):
            T.temporal_host(color, mom, **args)
        if "cam_cur" in kw or "cam_prev" in kw:
            assert T.camera(kw.get("cam_cur", kw.get("cam_prev")), 2, 2) is None      # the reference refuses the same cameras
    assert T.temporal_host(color, mom, 2, c, cam_prev=c, hist=h)[0] is not None


def test_the_stand_alone_program_runs_clean():
    """tests/temporal_host/temporal_host: the same functions behind a main of their own (the target of the sanitizer build,
    `make temporal_host_san`)"""
    d = os.path.join(T.HERE, "temporal_host")
    subprocess.check_call(["make", "-s", "-C", d, "temporal_host"])
    out = subprocess.run([os.path.join(d, "temporal_host")], capture_output=True, text=True)
    assert out.returncode == 0 and "temporal_host: ok" in out.stdout, out.stdout + out.stderr
