"""Inputs of the quality tests of temporal super-resolution: tests/temporal_quality.py's scene (scenes.synthetic_scene(2000, 3), PT_MIS,
depth 8, no anti-aliasing) from its LAST camera, at rest, whose 1024-spp picture at 48 x 48 is tests/golden/temporal_quality_ref_48x48.npy
-- the static camera of tests/upsample_quality.py.  Eight lo frames at 24 x 24 and 4 spp (4 colours, seed 7 + frame) from the CPU oracle,
once with the lo grid moved by jitter_sequence(8) (the camera sheared as the package's jittered_camera does) and once unjittered, and three
estimates of the picture from them:
  (A) the jittered frames accumulated into a 48 x 48 history by temporal_upsample_ref
  (B) the last jittered frame alone through upsample_ref with upsample_torch's shipped setting
  (C) the unjittered frames accumulated at 24 x 24 by temporal_ref and upsampled once with that setting"""
import json
import os

import numpy as np

import orc
import temporal_quality as Q
import upsample_quality as UQ

F = np.float32
W = H = 48
LW = LH = 24
FRAMES, SPP, SEED = 8, 4, 7
K = UQ.K
MAX_HISTORY = 64                    # 8 frames of 4 colours are never capped
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def lo_frame(art, k, jitter):
    """lo frame k on the CPU: (accum, moments, guides with id) of the oracle's samples under the camera sheared by `jitter` ((0, 0): as it is)"""
    import conv, hostsim, moments_ref
    import test_gpu_aov as aov
    sd = Q.scene(K)
    m = art.temporal_upsample.jittered_camera(np.array(list(sd.desc.cam_matrix), F), LW, jitter).reshape(-1)
    for j in range(16):
        sd.desc.cam_matrix[j] = float(m[j])
    osc = conv.OracleScene(sd)
    if "bvh" not in _cache:
        _cache["bvh"] = hostsim.bvh(art, sd)
    nodes, tris, info = _cache["bvh"]
    osc.attach_bvh(nodes, tris, info["width"])
    rad = moments_ref.sample_radiance(osc.scene, orc.make_params(LW, LH, orc.PT_MIS, False, Q.DEPTH, 1, seed=SEED + k), 0, SPP)
    acc, mom = moments_ref.add_colours(moments_ref.colours(rad, False))
    d = aov.camera_dirs(sd.desc, LW, LH, False)
    o = np.tile(np.array(list(sd.desc.cam_pos), F), (LW * LH, 1))
    raw = aov.host_raw(hostsim.trace(art, sd, o, np.ascontiguousarray(d.reshape(-1, 3)))[0]).reshape(LW * LH, 11)
    f, hit = raw.view(F), raw[:, 1] == 1
    table, _ = aov.albedo_table(art, sd.desc)
    guides = dict(albedo=np.where(hit[:, None], table[np.where(hit, raw[:, 5], 0)], F(0)).astype(F).reshape(LH, LW, 3),
                  normal=np.where(hit[:, None], f[:, 6:9], F(0)).astype(F).reshape(LH, LW, 3), depth=np.where(hit, f[:, 0], F(0)).astype(F).reshape(LH, LW),
                  id=np.where(hit, raw[:, 3], -1).astype(np.int32).reshape(LH, LW))
    return acc.astype(F), mom.astype(F), guides


def inputs(art):
    """(jitters [8, 2], the jittered lo frames, the unjittered lo frames, the hi guides), once per process"""
    if "inputs" not in _cache:
        jit = art.temporal_upsample.jitter_sequence(FRAMES)
        jittered = [lo_frame(art, k, (float(jit[k][0]), float(jit[k][1]))) for k in range(FRAMES)]
        plain = [lo_frame(art, k, (0.0, 0.0)) for k in range(FRAMES)]
        _, hi = UQ.cpu_frame(art, W, H, 0)
        _cache["inputs"] = (jit, jittered, plain, hi)
    return _cache["inputs"]


def demodulated(acc, albedo):
    """what INTEGRATION.md section 6l tells the caller to do before the call: the lo colour over the floored lo albedo"""
    return (acc / np.maximum(albedo, F(1e-3))).astype(F)


def chain_a(run, art, radius, min_confidence, demodulate, frames=FRAMES):
    """(A) through `run` (temporal_upsample_ref.temporal_upsample's signature): the picture after `frames` jittered frames"""
    jit, jittered, _, hi = inputs(art)
    cam = Q.camera(K)
    h, out = None, None
    for k in range(frames):
        acc, mom, g = jittered[k]
        c = demodulated(acc, g["albedo"]) if demodulate else acc
        res = run(lo_color=c, lo_moments=mom, n_colours=SPP, cam_cur=cam, cam_prev=cam if h is not None else None, hist=h, lo=g, hi=hi,
                  jitter=(float(jit[k][0]), float(jit[k][1])), radius=radius, min_confidence=min_confidence, max_history=MAX_HISTORY,
                  depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN, scale=1.0 / SPP)
        h, out = res[0], res[1]
    return (out * np.maximum(hi["albedo"], F(1e-3))).astype(F) if demodulate else out


def upsample_setting():
    b = UQ.record()["best"]
    names = ("albedo", "normal", "depth") + (("id",) if b["ids"] else ())
    return names, dict(footprint=b["footprint"], sigma_depth=b["sigma_depth"], normal_log2=b["normal_log2"], demodulate=b["demodulate"])


def chain_b(art):
    """(B): the last jittered lo frame alone, upsampled with upsample_torch's shipped setting"""
    import upsample_ref as U
    jit, jittered, _, hi = inputs(art)
    acc, _, g = jittered[-1]
    names, kw = upsample_setting()
    return U.upsample(acc, U.subset(g, names), U.subset(hi, names), scale=1.0 / SPP, jitter=(float(jit[-1][0]), float(jit[-1][1])), **kw)[0]


def chain_c(art):
    """(C): the unjittered lo frames accumulated at 24 x 24 by temporal_ref, upsampled once with the same setting"""
    import temporal_ref as T
    import upsample_ref as U
    _, _, plain, hi = inputs(art)
    cam = Q.camera(K)
    h, res = None, None
    for acc, mom, g in plain:
        res = T.temporal(acc, mom, SPP, cam, cam_prev=cam, hist=h, normal=g["normal"], depth=g["depth"], ids=g["id"], max_history=MAX_HISTORY,
                         depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN, scale=1.0 / SPP)
        h = res[0]
    names, kw = upsample_setting()
    g = plain[-1][2]
    return U.upsample(res[1], U.subset(g, names), U.subset(hi, names), scale=1.0, **kw)[0]


def reference():
    return Q.reference()


rms = Q.rms


def record():
    """the sweep's record (profiles/temporal_upsample/quality.json)"""
    with open(os.path.join(ROOT, "profiles", "temporal_upsample", "quality.json")) as f:
        return json.load(f)
