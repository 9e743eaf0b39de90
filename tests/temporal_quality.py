"""Inputs of the quality tests of temporal accumulation: scenes.synthetic_scene(2000, 3) at 48 x 48, PT_MIS, depth 8, no anti-aliasing,
four cameras along a small pan, 4 spp each (4 colours, seed 7 + frame), and the CPU oracle's 1024-spp picture of the LAST camera
(tests/golden/temporal_quality_ref_48x48.npy, written once by profiles/temporal/quality.py: the oracle's own estimator, seed 11)."""
import json
import os

import numpy as np

import orc

F = np.float32
W = H = 48
SPP, SEED, DEPTH, FRAMES = 4, 7, 8, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def camera(k):
    """(cam_pos, cam_matrix) of frame k: 0.05 to the right per frame, identity matrix"""
    return (np.array([0.05 * k, 2.55, 12.5], F), np.eye(4, dtype=F))


def scene(k):
    from ada_ray_tracer_amd import scenes
    sd = scenes.synthetic_scene(2000, 3)
    for j in range(3):
        sd.desc.cam_pos[j] = float(camera(k)[0][j])
    return sd


def reference():
    return np.load(os.path.join(orc.GOLDEN, "temporal_quality_ref_48x48.npy"))


def rms(x, ref):
    return float(np.sqrt(((np.asarray(x, np.float64) - ref) ** 2).mean()))


def shipped():
    """the sweep's record: the best setting and the ratio the numpy references reached with it (profiles/temporal/quality.json)"""
    with open(os.path.join(ROOT, "profiles", "temporal", "quality.json")) as f:
        return json.load(f)["best"]


def bound(best):
    """the asserted ratio: halfway between 1 and what the references reached in the sweep"""
    return 0.5 * (1.0 + best["ratio_filtered"])


def cpu_frame(art, k, reference_spp=0):
    """frame k on the CPU: (accum, moments, guides with prim_index) from the oracle's samples and the product's host build; with
    reference_spp also the oracle's picture of that camera at that many samples (seed 11)"""
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


def chain(frames, max_history, depth_tol, normal_min, iterations, sigma_color):
    """the numpy references over frames [(accum, moments, guides)] at camera(k): (last frame alone, after accumulation, after the filter)"""
    import svgf_var_ref as V
    import temporal_ref as T
    h, prev, res = None, None, None
    for k, (acc, mom, g) in enumerate(frames):
        res = T.temporal(acc, mom, SPP, camera(k), cam_prev=prev, hist=h, normal=g["normal"], depth=g["depth"], ids=g["prim_index"],
                         max_history=max_history, depth_tol=depth_tol, normal_min=normal_min, scale=1.0 / SPP)
        h, prev = res[0], camera(k)
    acc, mom, g = frames[-1]
    filt = V.denoise_var(res[1], res[2], albedo=g["albedo"], normal=g["normal"], depth=g["depth"], iterations=iterations, sigma_color=sigma_color)[0]
    return acc / F(SPP), res[1], filt
