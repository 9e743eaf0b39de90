"""Inputs of the quality tests of firefly suppression: the scene, size and pan of tests/temporal_quality.py (scenes.synthetic_scene(2000, 3)
at 48 x 48, PT_MIS, depth 8, no anti-aliasing, four cameras, seed 7 + frame) at a chosen spp from the CPU oracle through
tests/moments_ref.py, against the oracle's 1024-spp picture of the LAST camera (tests/golden/temporal_quality_ref_48x48.npy); the
planted spikes; and the chain firefly -> temporal accumulation over the pan, of any implementation of the two calls."""
import json
import os

import numpy as np

import orc
import temporal_quality as Q

F = np.float32
W, H, FRAMES, DEPTH, SEED = Q.W, Q.H, Q.FRAMES, Q.DEPTH, Q.SEED
LAST = FRAMES - 1
SPPS = (1, 4, 8)
ASSERTED_SPP = 4                         # the pan as tests/temporal_quality.py renders it
camera, scene, rms, reference = Q.camera, Q.scene, Q.rms, Q.reference
PLANTED, PLANT_FACTOR, PLANT_SEED = 12, 1000.0, 5
PLANT_SETTING = dict(radius=1, rank=1, gain=2.0)

_frames = {}


def cpu_frame(art, k, spp):
    """frame k on the CPU at spp colours: tests/temporal_quality.py's cpu_frame with the spp a parameter, once per process"""
    if (k, spp) in _frames:
        return _frames[k, spp]
    import conv, hostsim, moments_ref
    import test_gpu_aov as aov
    sd = scene(k)
    osc = conv.OracleScene(sd)
    nodes, tris, info = hostsim.bvh(art, sd)
    osc.attach_bvh(nodes, tris, info["width"])
    rad = moments_ref.sample_radiance(osc.scene, orc.make_params(W, H, orc.PT_MIS, False, DEPTH, 1, seed=SEED + k), 0, spp)
    acc, mom = moments_ref.add_colours(moments_ref.colours(rad, False))
    d = aov.camera_dirs(sd.desc, W, H, False)
    o = np.tile(np.array(list(sd.desc.cam_pos), F), (W * H, 1))
    raw = aov.host_raw(hostsim.trace(art, sd, o, np.ascontiguousarray(d.reshape(-1, 3)))[0]).reshape(W * H, 11)
    f, hit = raw.view(F), raw[:, 1] == 1
    guides = dict(normal=np.where(hit[:, None], f[:, 6:9], F(0)).astype(F).reshape(H, W, 3), depth=np.where(hit, f[:, 0], F(0)).astype(F).reshape(H, W),
                  prim_index=np.where(hit, raw[:, 3], -1).astype(np.int32).reshape(H, W))
    for a in (acc, mom) + tuple(guides.values()):
        a.setflags(write=False)
    _frames[k, spp] = (acc, mom.reshape(H, W, 2), guides)
    return _frames[k, spp]


def record():
    """the sweep's record (profiles/firefly/quality.json)"""
    with open(os.path.join(Q.ROOT, "profiles", "firefly", "quality.json")) as f:
        return json.load(f)


def mean_luminance(c):
    import firefly_ref as R
    return float(R.lum3(np.asarray(c, F)).astype(np.float64).mean())


def chain(art, frames, spp, firefly, temporal, setting=None):
    """the pan through `firefly` (firefly_ref.firefly's signature; setting None: the chain without the call) and `temporal`
    (temporal_ref.temporal's): per frame (the frame alone as the temporal step was given it, the history's colour, the flags or None)"""
    h, prev, res = None, None, []
    for k, (acc, mom, g) in enumerate(frames):
        flags = None
        if setting is None:
            color, moments, scale = acc, mom, 1.0 / spp
        else:
            ids = g["prim_index"] if setting.get("ids") else None
            color, moments, flags = firefly(acc, mom, ids, scale=1.0 / spp, **{n: v for n, v in setting.items() if n != "ids"})
            scale = 1.0
        r = temporal(color, moments, spp, camera(k), cam_prev=prev, hist=h, normal=g["normal"], depth=g["depth"], ids=g["prim_index"],
                     max_history=art.TEMPORAL_MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN, scale=scale)
        h, prev = r[0], camera(k)
        res.append(((F(scale) * np.asarray(color, F)).astype(F), r[1], flags))
    return res


def shipped(art):
    """firefly_torch's defaults as a setting of chain()"""
    fi = art.firefly
    return dict(radius=fi.FIREFLY_RADIUS, rank=fi.FIREFLY_RANK, gain=fi.FIREFLY_GAIN, floor=fi.FIREFLY_FLOOR, ids=False)


# ---- planted spikes ---------------------------------------------------------------------------------------------------------------
def plant(color, moments, scale, radius=1, seed=PLANT_SEED):
    """PLANTED pixels by a fixed seed, at least 3 apart (Chebyshev), at least `radius` from the border, not bad and not black, their colour
    and moments times PLANT_FACTOR: (colour, moments, [(y, x)]).  A pixel is passed over when the reference clamps one of its 8
    neighbours on the unplanted frame (a natural firefly next to it: the planted spike would raise that neighbour's limit and so change
    its words), or when it is so dark beside its neighbours that PLANT_FACTOR does not lift it over its limit."""
    import firefly_ref as R
    color, moments = np.array(color, F), np.array(moments, F).reshape(color.shape[0], color.shape[1], 2)
    Hh, Ww = color.shape[:2]
    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):
        l = R.lum3((F(scale) * color).astype(F))
    flagged = R.firefly(color, moments, None, scale=scale, **PLANT_SETTING)[2] == 1
    spots = []
    for i in rng.permutation(Hh * Ww):
        y, x = divmod(int(i), Ww)
        if not (radius <= y < Hh - radius and radius <= x < Ww - radius) or not (np.isfinite(color[y, x]).all() and np.isfinite(l[y, x]) and l[y, x] > 0):
            continue
        ring_l = np.delete(l[y - 1:y + 2, x - 1:x + 2].reshape(-1), 4)
        ring_l = ring_l[np.isfinite(ring_l)]
        if flagged[y - 1:y + 2, x - 1:x + 2].sum() > int(flagged[y, x]) or ring_l.size == 0 or not (0.5 * PLANT_FACTOR * l[y, x] > 2.0 * PLANT_SETTING["gain"] * ring_l.max()):
            continue
        if all(max(abs(y - v), abs(x - u)) >= 3 for v, u in spots):
            spots.append((y, x))
        if len(spots) == PLANTED:
            break
    assert len(spots) == PLANTED
    for y, x in spots:
        color[y, x] *= F(PLANT_FACTOR)
        moments[y, x] *= F(PLANT_FACTOR)
    return color, moments, spots


def check_planted(run, color, moments, scale):
    """of any implementation with firefly_ref.firefly's signature, over one frame: every planted pixel is flagged 1 (the share that may
    be missed is 0); the 8 neighbours of a planted pixel keep the words they get from the unplanted frame; and outside the planted
    pixels and their neighbours exactly the pixels flagged on the unplanted frame are flagged"""
    import firefly_ref as R
    pc, pm, spots = plant(color, moments, scale)
    kw = dict(scale=scale, **PLANT_SETTING)
    base, got = run(color, moments, None, **kw), run(pc, pm, None, **kw)
    ys, xs = np.array(spots).T
    assert (got[2][ys, xs] == 1).all(), "planted pixels missed: %d of %d" % (int((got[2][ys, xs] != 1).sum()), PLANTED)
    near = np.zeros(got[2].shape, bool)
    for y, x in spots:
        near[y - 1:y + 2, x - 1:x + 2] = True
    ring = near.copy(); ring[ys, xs] = False
    assert ring.sum() == 8 * PLANTED
    assert R.differ(got[0][ring], base[0][ring]) == 0 and R.differ(got[1][ring], base[1][ring]) == 0 and R.differ(got[2][ring], base[2][ring]) == 0
    assert ((got[2] != 0) == (base[2] != 0))[~near].all() and R.differ(got[0][~near], base[0][~near]) == 0
    # a planted pixel comes down to its limit: at most gain times its largest neighbour, never above what was planted
    with np.errstate(all="ignore"):
        assert (R.lum3(got[0])[ys, xs] < R.lum3((F(scale) * pc).astype(F))[ys, xs]).all()
    return got
