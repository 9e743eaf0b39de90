"""Rebuilding the instance tree of a moved instanced scene on the MI355X: art_rebuild_instance_tree_device against the art_upload_scene
it replaces (the only way to a new instance tree before the call existed), and what the new tree is worth to the rays.

For I64 (scenes.instanced_scene(): 64 instances x 20 k triangles, the scene of bench.py --scene i64) and I4096 (4096 instances x 300
triangles of the same two meshes), default options.  The instances scatter: the translations are permuted among them.
  upload_wall_ms      wall time of art_upload_scene of the scattered scene (host trees, host instance tree, copies), median of 5
  rebuild_wall_ms     wall time of rebuild_instances() after the move, median of 5 (a move back and forth between them, untimed)
  host_ms, gather_ms, build_ms     ArtInstanceRebuildInfo per rebuild, from the differences of the cumulative figures: medians of the same 5
  cost                instance_tree_cost() of the moved tree and of the rebuilt one
  mrays               Mrays/s of a fixed set of random rays (trace_rays_torch, median of 5 timed launches after one warm launch, HIP
                      events through torch) through the moved tree and through the rebuilt one
Every figure comes from one process; the caller runs this script under a time limit of its own.

usage: python profiles/rebuild_instances/measure.py --out DIR [--scenes i64,i4096] [--rays 1048576]
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


def mats(sd):
    return np.array([list(sd.desc.instances[i].m) for i in range(sd.desc.n_instances)], np.float32).reshape(-1, 3, 4)


def cost(be):
    c = be.instance_tree_cost()
    return {"root_area": c.root_area, "node_visits": c.node_visits, "leaf_visits": c.leaf_visits}


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
    out = {"what": "art_rebuild_instance_tree_device against art_upload_scene of the scattered scene; rays through the moved and the rebuilt instance tree",
           "device": torch.cuda.get_device_name(0), "cases": []}
    rng = np.random.default_rng(5)
    n = args.rays
    o = torch.from_numpy((rng.random((n, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2]).astype(np.float32)).cuda()
    d = rng.normal(size=(n, 3)); d = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).cuda()
    for scene in args.scenes.split(","):
        ni, nt = (64, 20000) if scene == "i64" else (4096, 300)
        sd = scenes.instanced_scene(ni, nt)
        m0 = mats(sd)
        mesh = [int(sd.desc.instances[i].mesh) for i in range(ni)]
        perm = m0.copy(); perm[:, :, 3] = m0[rng.permutation(ni), :, 3]
        scattered = scenes.instanced_scene(0, nt, transforms=[(mesh[i], perm[i]) for i in range(ni)])
        case = {"scene": scene, "instances": ni, "triangles_per_mesh": nt}
        be.upload_scene(scattered)                                        # warm
        ups = []
        for _ in range(5):
            t0 = time.perf_counter(); be.upload_scene(scattered); ups.append((time.perf_counter() - t0) * 1e3)
        case["upload_wall_ms"] = statistics.median(ups); case["upload_wall_ms_runs"] = ups
        case["cost_fresh_upload"] = cost(be); case["mrays_fresh_upload"] = mrays(torch, be, o, d)
        be.upload_scene(sd)
        g0, g1 = torch.from_numpy(m0.copy()).cuda(), torch.from_numpy(perm.copy()).cuda()
        be.move_instances_torch(g1, check=False); torch.cuda.synchronize()
        case["entry_points"] = int(be.export_two_level()["inst"].shape[0])
        case["cost_moved"] = cost(be); case["mrays_moved"] = mrays(torch, be, o, d)
        be.rebuild_instances(); be.move_instances_torch(g0, check=False)  # warm: the first rebuild loads the builder's code
        wall, host, gather, build = [], [], [], []
        for _ in range(5):
            be.rebuild_instances(); be.move_instances_torch(g1, check=False); torch.cuda.synchronize()      # a tree built for the home placement, moved
            before = be.instance_rebuild_info()
            t0 = time.perf_counter(); be.rebuild_instances(); wall.append((time.perf_counter() - t0) * 1e3)
            after = be.instance_rebuild_info()
            host.append(after.host_ms - before.host_ms); gather.append(after.gather_ms - before.gather_ms); build.append(after.build_ms - before.build_ms)
            if len(wall) < 5:
                be.move_instances_torch(g0, check=False)
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
    ap.add_argument("--scenes", default="i64,i4096")
    ap.add_argument("--rays", type=int, default=1 << 20)
    measure(ap.parse_args())
