"""The cost of moving geometry on the MI355X: art_refit_device against the art_upload_scene it replaces.

For scenes C4 (1 M random triangles) and S4 (1 M structured triangles), default build (GPU binned SAH, width 4):
  plan_ms             host time of the first refit's plan (nodes grouped by depth, scratch), ArtRefitInfo.plan_ms
  first_refit_wall_ms wall time of the first refit_torch + torch.cuda.synchronize() (plan included)
  refit_ms            GPU time of one refit's kernels (HIP events, ArtRefitInfo.refit_ms), median over 20 refits
  refit_wall_ms       wall time of one refit_torch(check=False) + synchronize, median over the same 20 refits
  refit_checked_wall_ms  the same with check=True (one host synchronisation inside refit_torch), median of 5
  upload_ms           wall time of art_upload_scene of the moved mesh (host flattening, copies, GPU build), median of 3
  visits_per_ray      node visits per ray (count_tests, art_trace_rays with stats) of 1 M random rays: the uploaded tree, the tree refitted
                      to a moderate deformation, and a fresh build of the deformed mesh
  trace_ms_per_launch trace kernel time per launch of a 640 x 480 PT_MIS render on the unmoved scene, before any refit and after a refit
                      to the uploaded positions (the same tree bytes: the render path must not change)

usage: python profiles/refit/measure.py --out DIR [--scenes c4,s4]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def deform(pos):
    """A moderate, smooth deformation: a 0.2 rad turn about the vertical axis through the centre plus a displacement of up to 0.1."""
    p = pos.astype(np.float64)
    c = p.mean(0)
    a = 0.2
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    q = (p - c) @ R.T + c
    q += 0.1 * np.stack([np.sin(2.0 * q[:, 1]), np.sin(2.0 * q[:, 2]), np.sin(2.0 * q[:, 0])], 1)
    return q.astype(np.float32)


def visits(be, o, d):
    _, st = be.trace_rays(o, d, want_stats=True)
    return st.node_visits / max(1, st.traced_rays)


def trace_ms_per_launch(art, be):
    be.resize(640, 480)
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=11)
    spp = 0
    for _ in range(3):
        _, _, spp = be.render_pass(p, spp, False, False)
    st = be.stats()
    return st.trace_ms / max(1, st.trace_launches)


def measure(args):
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    out = {"what": "art_refit_device against art_upload_scene of the moved mesh", "device": torch.cuda.get_device_name(0), "cases": []}
    rng = np.random.default_rng(5)
    n = 1 << 20
    o = (rng.random((n, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2]).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    for scene in args.scenes.split(","):
        sd = scenes.synthetic_scene(1000000, 4) if scene == "c4" else scenes.structured_scene(1000000)
        pos, nrm, idx, _, matid = sd._mesh_arrays[-1]
        p2 = deform(pos)
        moved = art.SceneDesc(meshes=[dict(mode=art.MESH_CLOSEST, pos=p2, nrm=nrm, idx=idx, matid=matid)], **sd._kw)
        case = {"scene": scene, "triangles": int(idx.shape[0]), "vertices": int(pos.shape[0])}
        be.upload_scene(sd)
        case["trace_ms_per_launch_before"] = trace_ms_per_launch(art, be)
        case["visits_per_ray_uploaded"] = visits(be, o, d)
        pg, p2g = torch.from_numpy(pos).cuda(), torch.from_numpy(p2).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); be.refit_torch(pg, check=False); torch.cuda.synchronize()
        case["first_refit_wall_ms"] = (time.perf_counter() - t0) * 1e3
        case["plan_ms"] = be.refit_info().plan_ms
        case["trace_ms_per_launch_after_identity_refit"] = trace_ms_per_launch(art, be)
        ms, wall, wall_checked = [], [], []
        for k in range(20):
            before = be.refit_info().refit_ms
            t0 = time.perf_counter(); be.refit_torch(p2g if k % 2 == 0 else pg, check=False); torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(be.refit_info().refit_ms - before)
        for k in range(5):
            t0 = time.perf_counter(); be.refit_torch(p2g if k % 2 == 0 else pg); torch.cuda.synchronize()
            wall_checked.append((time.perf_counter() - t0) * 1e3)
        case["refit_ms"] = statistics.median(ms); case["refit_ms_runs"] = ms
        case["refit_wall_ms"] = statistics.median(wall)
        case["refit_checked_wall_ms"] = statistics.median(wall_checked)
        be.refit_torch(p2g); torch.cuda.synchronize()
        case["visits_per_ray_refitted"] = visits(be, o, d)
        ups = []
        for _ in range(3):
            t0 = time.perf_counter(); be.upload_scene(moved); ups.append((time.perf_counter() - t0) * 1e3)
        case["upload_ms"] = statistics.median(ups); case["upload_ms_runs"] = ups
        case["gpu_build_ms"] = be.bvh_info().build_ms
        case["visits_per_ray_rebuilt"] = visits(be, o, d)
        case["upload_over_refit_wall"] = case["upload_ms"] / case["refit_wall_ms"]
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        del pg, p2g
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "measure.json"), "w") as f:
        json.dump(out, f, indent=1)
    be.shutdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="output directory of measure.json")
    ap.add_argument("--scenes", default="c4,s4")
    measure(ap.parse_args())
