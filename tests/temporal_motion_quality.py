"""Inputs and sweep of the quality tests of temporal accumulation that follows a moving mesh: the Cornell box of scenes.synthetic_scene
with a small torus (80 triangles, the scene's CLOSEST mesh) in place of the soup, 48 x 48, PT_MIS, depth 8, no anti-aliasing, the
camera at rest.  The torus moves parallel to the image plane, 0.75 to the right per frame (about two pixels); four frames at 4 spp each
(4 colours, seed 7 + frame) come from the CPU oracle -- each pose is simply another scene to it -- and the truth is the oracle's
1024-spp picture of the LAST pose (tests/golden/motion_quality_ref_48x48.npy, written once by `python tests/temporal_motion_quality.py
--golden`: the oracle's own estimator, seed 11).  Run as a program it computes the figures the tests assert, with the numpy references
only, and writes them to profiles/motion/quality.json."""
import json
import os
import sys

import numpy as np

F = np.float32
W = H = 48
SPP, SEED, DEPTH, FRAMES = 4, 7, 8, 4
STEP = 0.75                                   # world units per frame along x: about two pixels at the torus' distance
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JSON = os.path.join(ROOT, "profiles", "motion", "quality.json")
CAMERA = (np.array([0.0, 2.55, 12.5], F), np.eye(4, dtype=F))


def mesh(k):
    """the torus at pose k: positions translated in binary32 from pose 0, the arrays a refit is given"""
    from ada_ray_tracer_amd import scenes
    m = scenes.torus_mesh(nu=10, nv=4, R=0.9, r=0.45, centre=(-1.1, 2.2, 3.0))
    m["pos"] = (m["pos"] + np.array([STEP * k, 0.0, 0.0], F)).astype(F)
    return m


def scene(k):
    from ada_ray_tracer_amd import scenes
    import ada_ray_tracer_amd as art
    base = scenes.synthetic_scene(2, 3)
    return art.SceneDesc(meshes=[mesh(k)], **base._kw)


def reference():
    import orc
    return np.load(os.path.join(orc.GOLDEN, "motion_quality_ref_48x48.npy"))


def rms(x, ref, mask):
    d = (np.asarray(x, np.float64) - ref)[mask]
    return float(np.sqrt((d ** 2).mean()))


def record():
    with open(JSON) as f:
        return json.load(f)


def cpu_frame(art, k, reference_spp=0):
    """frame k on the CPU: (accum, moments, guides with prim_type, prim_index and motion) from the oracle's samples and the product's
    host build; with reference_spp also the oracle's picture of that pose at that many samples (seed 11)"""
    import conv, hostsim, moments_ref, orc
    import motion_ref as M
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
    cur, prev = mesh(k), mesh(max(k - 1, 0))
    motion = M.from_hits(raw.reshape(1, -1, 11), d, CAMERA[0], idx=cur["idx"], cur=cur["pos"], prev=prev["pos"])
    guides = dict(albedo=np.where(hit[:, None], table[np.where(hit, raw[:, 5], 0)], F(0)).astype(F).reshape(H, W, 3),
                  normal=np.where(hit[:, None], f[:, 6:9], F(0)).astype(F).reshape(H, W, 3), depth=np.where(hit, f[:, 0], F(0)).astype(F).reshape(H, W),
                  prim_index=np.where(hit, raw[:, 3], -1).astype(np.int32).reshape(H, W), prim_type=np.where(hit, raw[:, 2], -1).astype(np.int32).reshape(H, W),
                  motion=motion.reshape(H, W, 3))
    ref = None
    if reference_spp:
        ref, rspp, _ = orc.render(osc.scene, orc.make_params(W, H, orc.PT_MIS, False, DEPTH, 64, seed=11), passes=reference_spp // 64)
        ref = (ref / F(rspp)).astype(F)
    return acc, mom, guides, ref


def chain(frames, with_motion, max_history, depth_tol, normal_min):
    """the numpy reference over frames [(accum, moments, guides)]: (the last frame's colour, [history length after each frame])"""
    import temporal_motion_ref as TM
    h, res, lengths = None, None, []
    for k, (acc, mom, g) in enumerate(frames):
        res = TM.temporal(acc, mom, SPP, CAMERA, cam_prev=CAMERA if k else None, hist=h, normal=g["normal"], depth=g["depth"], ids=g["prim_index"],
                          max_history=max_history, depth_tol=depth_tol, normal_min=normal_min, scale=1.0 / SPP, motion=g["motion"] if with_motion else None)
        h = res[0]
        lengths.append(res[3])
    return res[1], lengths


def figures(frames, ref, max_history, depth_tol, normal_min):
    """what the tests assert, from the frames' planes (the CPU's or the GPU's) and the truth"""
    acc, mom, g = frames[-1]
    on = g["prim_type"] == 2                       # ray 0 hits the mesh in the last frame
    last = acc / F(SPP)
    cam_col, cam_len = chain(frames, False, max_history, depth_tol, normal_min)
    mo_col, mo_len = chain(frames, True, max_history, depth_tol, normal_min)
    on_k = [f[2]["prim_type"] == 2 for f in frames]
    out = dict(mesh_pixels=int(on.sum()),
               mesh=dict(before=rms(last, ref, on), camera_only=rms(cam_col, ref, on), after=rms(mo_col, ref, on)),
               rest=dict(before=rms(last, ref, ~on), camera_only=rms(cam_col, ref, ~on), after=rms(mo_col, ref, ~on)),
               mean_length_mesh_camera_only=[float(l[m].mean()) for l, m in zip(cam_len, on_k)],
               mean_length_mesh_motion=[float(l[m].mean()) for l, m in zip(mo_len, on_k)],
               restarted_share_mesh_frame2=float((mo_len[1][on_k[1]] <= SPP).mean()))
    out["ratio"] = out["mesh"]["after"] / out["mesh"]["before"]
    return out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import orc
    art = ge.load_package()
    if "--golden" in sys.argv:
        np.save(os.path.join(orc.GOLDEN, "motion_quality_ref_48x48.npy"), cpu_frame(art, FRAMES - 1, reference_spp=1024)[3])
    frames = [cpu_frame(art, k)[:3] for k in range(FRAMES)]
    kw = dict(max_history=art.TEMPORAL_MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN)
    fig = figures(frames, reference(), **kw)
    fig["settings"] = kw
    fig["bound"] = 0.5 * (1.0 + fig["ratio"])       # the asserted ratio r: halfway between 1 and what the references reached
    os.makedirs(os.path.dirname(JSON), exist_ok=True)
    with open(JSON, "w") as f:
        json.dump(fig, f, indent=1)
        f.write("\n")
    print(json.dumps(fig, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
