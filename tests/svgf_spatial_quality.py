"""Inputs of the quality tests of the spatial variance estimate: the scene, size and pan of tests/temporal_quality.py at ONE colour per
frame -- no anti-aliasing, 1 spp per frame (seed 7 + frame) from the CPU oracle through tests/moments_ref.py -- and the oracle's 1024-spp
pictures of the SECOND and the LAST camera (tests/golden/svgf_spatial_quality_ref_48x48.npy, [2, 48, 48, 3], written once by
profiles/svgf_spatial/quality.py: the oracle's own estimator, seed 11).  The second frame is where every history is short."""
import json
import os

import numpy as np

import orc
import temporal_quality as Q

F = np.float32
W, H, FRAMES, DEPTH, SEED = Q.W, Q.H, Q.FRAMES, Q.DEPTH, Q.SEED
SPP = 1                                  # one colour per frame
SECOND, LAST = 1, FRAMES - 1
camera, scene, rms = Q.camera, Q.scene, Q.rms


def reference():
    """(the second camera's picture, the last camera's)"""
    r = np.load(os.path.join(orc.GOLDEN, "svgf_spatial_quality_ref_48x48.npy"))
    return r[0], r[1]


def shipped():
    """the sweep's record (profiles/svgf_spatial/quality.json)"""
    with open(os.path.join(Q.ROOT, "profiles", "svgf_spatial", "quality.json")) as f:
        return json.load(f)


def bound(ratio):
    """the asserted ratio: halfway between 1 and what the references reached in the sweep"""
    return 0.5 * (1.0 + ratio)


def cpu_frame(art, k, reference_spp=0):
    """frame k on the CPU: tests/temporal_quality.py's cpu_frame at 1 spp"""
    import conv, hostsim, moments_ref
    import test_gpu_aov as aov
    sd = scene(k)
    osc = conv.OracleScene(sd)
    nodes, tris, info = hostsim.bvh(art, sd)
    osc.attach_bvh(nodes, tris, info["width"])
    rad = moments_ref.sample_radiance(osc.scene, orc.make_params(W, H, orc.PT_MIS, False, DEPTH, 1, seed=SEED + k), 0, SPP)
    acc, mom = moments_ref.add_colours(moments_ref.colours(rad, False))
    d = aov.camera_dirs(sd.desc, W, H, False)
    o = np.tile(np.array(list(sd.desc.cam_pos), F), (W * H, 1))
    raw = aov.host_raw(hostsim.trace(art, sd, o, np.ascontiguousarray(d.reshape(-1, 3)))[0]).reshape(W * H, 11)
    f, hit = raw.view(F), raw[:, 1] == 1
    table, _ = aov.albedo_table(art, sd.desc)
    guides = dict(albedo=np.where(hit[:, None], table[np.where(hit, raw[:, 5], 0)], F(0)).astype(F).reshape(H, W, 3),
                  normal=np.where(hit[:, None], f[:, 6:9], F(0)).astype(F).reshape(H, W, 3), depth=np.where(hit, f[:, 0], F(0)).astype(F).reshape(H, W),
                  prim_index=np.where(hit, raw[:, 3], -1).astype(np.int32).reshape(H, W))
    ref = None
    if reference_spp:
        ref, rspp, _ = orc.render(osc.scene, orc.make_params(W, H, orc.PT_MIS, False, DEPTH, 64, seed=11), passes=reference_spp // 64)
        ref = (ref / F(rspp)).astype(F)
    return acc, mom, guides, ref


def accumulate(art, frames):
    """art_temporal_device's reference over the frames with the shipped defaults: per frame (out, variance, history, guides)"""
    import temporal_ref as T
    h, prev, res = None, None, []
    for k, (acc, mom, g) in enumerate(frames):
        r = T.temporal(acc, mom, SPP, camera(k), cam_prev=prev, hist=h, normal=g["normal"], depth=g["depth"], ids=g["prim_index"],
                       max_history=art.TEMPORAL_MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN, scale=1.0 / SPP)
        h, prev = r[0], camera(k)
        res.append((r[1], r[2], r[0], g))
    return res


def filtered(step, iterations, sigma_color, spatial=None):
    """one accumulated frame through the variance-plane filter; spatial: None (the chain without the new call) or the keyword arguments
    of svgf_spatial_ref.spatial"""
    import svgf_spatial_ref as SP
    import svgf_var_ref as V
    out, var, hist, g = step
    if spatial is not None:
        var = SP.spatial(hist, var, **spatial)
    return V.denoise_var(out, var, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], iterations=iterations, sigma_color=sigma_color)[0], var
