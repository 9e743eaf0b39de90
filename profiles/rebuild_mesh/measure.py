"""Rebuilding one mesh's tree of an instanced scene on the MI355X: art_rebuild_mesh_tree_device against the art_upload_scene it
replaces (the only way to a new mesh tree before the call existed), and what the new tree is worth to the rays.

For I64 (scenes.instanced_scene(): 64 instances of two 20 k-triangle meshes) and M1 (4 instances of two 1 M-triangle meshes), default
options but inst_open 1 (an opened instance of the mesh refuses the call).  Mesh 0 is warped inside its own box (u -> u ^ 6 per axis).
  upload_wall_ms      wall time of art_upload_scene of the deformed scene, median of 5
  rebuild_wall_ms     wall time of rebuild_mesh(0) after the refit, median of 5 (a refit back, a rebuild and the refit between them, untimed)
  host_ms, gather_ms, build_ms     ArtMeshRebuildInfo per rebuild, from the differences of the cumulative figures: medians of the same 5
  cost                mesh_tree_cost(0) of the refitted tree, the rebuilt one and the fresh upload's
  mrays               Mrays/s of a fixed set of random rays (trace_rays_torch, median of 5 timed launches after one warm launch, HIP
                      events through torch) through the three trees
Every figure comes from one process; the caller runs this script under a time limit of its own.

usage: python profiles/rebuild_mesh/measure.py --out DIR [--scenes i64,m1] [--rays 1048576]
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


def cost(be):
    c = be.mesh_tree_cost(0)
    return {"root_area": c.root_area, "node_visits": c.node_visits, "leaf_visits": c.leaf_visits, "tri_tests": c.tri_tests}


def mrays(torch, be, o, d):
    be.trace_rays_torch(o, d); torch.cuda.synchronize()                   # warm
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); be.trace_rays_torch(o, d); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return o.shape[0] / statistics.median(ms) / 1e3


def measure(args):
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    be.set_option("inst_open", 1)
    out = {"what": "art_rebuild_mesh_tree_device against art_upload_scene of the deformed scene; rays through the refitted, the rebuilt and the freshly uploaded tree",
           "device": torch.cuda.get_device_name(0), "cases": []}
    rng = np.random.default_rng(5)
    n = args.rays
    o = torch.from_numpy((rng.random((n, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2]).astype(np.float32)).cuda()
    d = rng.normal(size=(n, 3)); d = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).cuda()
    for scene in args.scenes.split(","):
        ni, nt = (64, 20000) if scene == "i64" else (4, 1000000)
        sd = scenes.instanced_scene(ni, nt)
        ms = []
        for k, (pos, nrm, idx, uv, matid) in enumerate(sd._mesh_arrays):
            p = np.asarray(pos, np.float32)
            if k == 0:
                p0 = p.copy()
                lo, hi = p.min(0), p.max(0)
                p = (lo + (hi - lo) * ((p - lo) / (hi - lo)) ** np.float32(6.0)).astype(np.float32)
                p1 = p
            ms.append(dict(mode=art.MESH_CLOSEST, pos=p, nrm=nrm, idx=idx, uv=uv, matid=matid))
        inst = [(int(sd.desc.instances[i].mesh), list(sd.desc.instances[i].m)) for i in range(sd.desc.n_instances)]
        deformed = art.SceneDesc(meshes=ms, instances=inst, **sd._kw)
        case = {"scene": scene, "instances": ni, "triangles_per_mesh": int(sd._mesh_arrays[0][2].shape[0])}
        be.upload_scene(deformed)                                         # warm
        ups = []
        for _ in range(5):
            t0 = time.perf_counter(); be.upload_scene(deformed); ups.append((time.perf_counter() - t0) * 1e3)
        case["upload_wall_ms"] = statistics.median(ups); case["upload_wall_ms_runs"] = ups
        case["cost_fresh_upload"] = cost(be); case["mrays_fresh_upload"] = mrays(torch, be, o, d)
        be.upload_scene(sd)
        g0, g1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
        be.refit_mesh_torch(0, g1, check=False); torch.cuda.synchronize()
        case["cost_refitted"] = cost(be); case["mrays_refitted"] = mrays(torch, be, o, d)
        be.rebuild_mesh(0)                                                # warm: the first rebuild loads the builder's code
        wall, host, gather, build = [], [], [], []
        for _ in range(5):
            be.refit_mesh_torch(0, g0, check=False); be.rebuild_mesh(0); be.refit_mesh_torch(0, g1, check=False); torch.cuda.synchronize()      # a tree built for the uploaded shape, refitted
            before = be.mesh_rebuild_info()
            t0 = time.perf_counter(); be.rebuild_mesh(0); wall.append((time.perf_counter() - t0) * 1e3)
            after = be.mesh_rebuild_info()
            host.append(after.host_ms - before.host_ms); gather.append(after.gather_ms - before.gather_ms); build.append(after.build_ms - before.build_ms)
        case["rebuild_wall_ms"] = statistics.median(wall); case["rebuild_wall_ms_runs"] = wall
        case["host_ms"] = statistics.median(host); case["gather_ms"] = statistics.median(gather); case["build_ms"] = statistics.median(build)
        case["cost_rebuilt"] = cost(be); case["mrays_rebuilt"] = mrays(torch, be, o, d)
        case["upload_over_rebuild_wall"] = case["upload_wall_ms"] / case["rebuild_wall_ms"]
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        del g0, g1
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "measure.json"), "w") as f:
        json.dump(out, f, indent=1)
    be.shutdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="output directory of measure.json")
    ap.add_argument("--scenes", default="i64,m1")
    ap.add_argument("--rays", type=int, default=1 << 20)
    measure(ap.parse_args())
