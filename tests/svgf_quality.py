"""Inputs of the quality tests of the variance-guided denoiser: the frame of profiles/svgf/quality.py (scenes.synthetic_scene(2000, 3),
48 x 48, PT_MIS, depth 8, no anti-aliasing, seed 7) and its 1024-spp reference picture, which that script wrote once
(tests/golden/svgf_quality_ref_48x48.npy: the CPU oracle's own estimator, seed 11)."""
import os

import numpy as np

import orc

F = np.float32
W = H = 48
SPP, SEED, DEPTH = 8, 7, 8


def reference():
    return np.load(os.path.join(orc.GOLDEN, "svgf_quality_ref_48x48.npy"))


def rms(x, ref):
    return float(np.sqrt(((np.asarray(x, np.float64) - ref) ** 2).mean()))


def scene():
    from ada_ray_tracer_amd import scenes
    return scenes.synthetic_scene(2000, 3)


def cpu_inputs(art):
    """(accum, moments, guides) of the 8-spp frame on the CPU: the oracle's samples through tests/moments_ref.py, the first hits of the
    pixel centres through the product's host build"""
    import conv, hostsim, moments_ref
    import test_gpu_aov as aov
    sd = scene()
    osc = conv.OracleScene(sd)
    nodes, tris, info = hostsim.bvh(art, sd)
    osc.attach_bvh(nodes, tris, info["width"])
    rad = moments_ref.sample_radiance(osc.scene, orc.make_params(W, H, orc.PT_MIS, False, DEPTH, 1, seed=SEED), 0, SPP)
    acc, mom = moments_ref.add_colours(moments_ref.colours(rad, False))
    d = aov.camera_dirs(sd.desc, W, H, False)
    o = np.tile(np.array(list(sd.desc.cam_pos), F), (W * H, 1))
    raw = aov.host_raw(hostsim.trace(art, sd, o, np.ascontiguousarray(d.reshape(-1, 3)))[0]).reshape(W * H, 11)
    f, hit = raw.view(F), raw[:, 1] == 1
    table, _ = aov.albedo_table(art, sd.desc)
    guides = dict(albedo=np.where(hit[:, None], table[np.where(hit, raw[:, 5], 0)], F(0)).astype(F).reshape(H, W, 3),
                  normal=np.where(hit[:, None], f[:, 6:9], F(0)).astype(F).reshape(H, W, 3), depth=np.where(hit, f[:, 0], F(0)).astype(F).reshape(H, W))
    return acc, mom, guides
