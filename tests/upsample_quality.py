"""Inputs of the quality tests of guided upsampling: tests/temporal_quality.py's scene (scenes.synthetic_scene(2000, 3), PT_MIS, depth 8, no
anti-aliasing) from its LAST camera, whose 1024-spp picture at 48 x 48 is tests/golden/temporal_quality_ref_48x48.npy (the CPU oracle's own
estimator, seed 11).  Three estimates of that picture at one ray budget: (a) 24 x 24 at 16 spp upsampled under the feature buffers of
both resolutions, (b) the same lo frame upsampled with no guide, (c) 48 x 48 at 4 spp."""
import json
import os

import numpy as np

import orc
import temporal_quality as Q

F = np.float32
W = H = 48
LW = LH = 24
LO_SPP, HI_SPP, SEED = 16, 4, 7
K = Q.FRAMES - 1                    # the camera of the golden picture
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_frame(art, w, h, spp):
    """the frame at w x h on the CPU: (mean colour or None with spp = 0, guides with id) from the oracle's samples and the product's host build"""
    import conv, hostsim, moments_ref
    import test_gpu_aov as aov
    sd = Q.scene(K)
    osc = conv.OracleScene(sd)
    nodes, tris, info = hostsim.bvh(art, sd)
    osc.attach_bvh(nodes, tris, info["width"])
    mean = None
    if spp:
        rad = moments_ref.sample_radiance(osc.scene, orc.make_params(w, h, orc.PT_MIS, False, Q.DEPTH, 1, seed=SEED), 0, spp)
        mean = (moments_ref.add_colours(moments_ref.colours(rad, False))[0] / F(spp)).astype(F)
    d = aov.camera_dirs(sd.desc, w, h, False)
    o = np.tile(np.array(list(sd.desc.cam_pos), F), (w * h, 1))
    raw = aov.host_raw(hostsim.trace(art, sd, o, np.ascontiguousarray(d.reshape(-1, 3)))[0]).reshape(w * h, 11)
    f, hit = raw.view(F), raw[:, 1] == 1
    table, _ = aov.albedo_table(art, sd.desc)
    guides = dict(albedo=np.where(hit[:, None], table[np.where(hit, raw[:, 5], 0)], F(0)).astype(F).reshape(h, w, 3),
                  normal=np.where(hit[:, None], f[:, 6:9], F(0)).astype(F).reshape(h, w, 3), depth=np.where(hit, f[:, 0], F(0)).astype(F).reshape(h, w),
                  id=np.where(hit, raw[:, 3], -1).astype(np.int32).reshape(h, w))
    return mean, guides


def reference():
    return Q.reference()


rms = Q.rms


def record():
    """the sweep's record (profiles/upsample/quality.json)"""
    with open(os.path.join(ROOT, "profiles", "upsample", "quality.json")) as f:
        return json.load(f)
