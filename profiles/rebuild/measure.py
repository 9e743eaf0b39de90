"""A new tree without leaving the GPU, on the MI355X: art_rebuild_device against the art_upload_scene it replaces, and how well the
tree-cost figure (art_get_tree_cost) predicts what a refitted tree costs in measured node visits.

For scenes C4 (1 M random triangles) and S4 (1 M structured triangles), default build (GPU binned SAH, width 4):
  rebuild_wall_ms     wall time of rebuild_torch(pos) (the call returns when the tree is committed) + torch.cuda.synchronize(), median of 7,
                      alternating with the uploads below in the same process
  rebuild_gather_ms / rebuild_build_ms / rebuild_host_ms   ArtRebuildInfo per rebuild: HIP events around the gather kernel, around the
                      build, host time inside the call; medians of the same 7
  upload_wall_ms      wall time of art_upload_scene of the same moved mesh (host flattening, copies, GPU build), median of 7
  upload_build_ms     ArtBvhInfo.build_ms of those uploads (HIP events around the same builder)
  upload_over_rebuild upload_wall_ms / rebuild_wall_ms
  same_tree           the rebuilt tree's export equals the upload's byte for byte
  sweep               for each deformation amount (1.0 = the deformation of profiles/refit/measure.py): tree_cost() and the node visits per
                      ray (count_tests, 1 M random rays through art_trace_rays) of the tree refitted to the moved mesh and of the tree
                      rebuilt for it, and the two ratios refitted / rebuilt

usage: python profiles/rebuild/measure.py --out DIR [--scenes c4,s4] [--amounts 0.25,0.5,1,2] [--triangles 1000000]
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


def deform(pos, amount=1.0):
    """amount x the deformation of profiles/refit/measure.py: a 0.2 rad turn about the vertical axis through the centre plus a smooth
    displacement of up to 0.1."""
    p = pos.astype(np.float64)
    c = p.mean(0)
    a = 0.2 * amount
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    q = (p - c) @ R.T + c
    q += 0.1 * amount * np.stack([np.sin(2.0 * q[:, 1]), np.sin(2.0 * q[:, 2]), np.sin(2.0 * q[:, 0])], 1)
    return q.astype(np.float32)


def visits(be, o, d):
    _, st = be.trace_rays(o, d, want_stats=True)
    return st.node_visits / max(1, st.traced_rays)


def cost(be):
    tc = be.tree_cost()
    return {"root_area": tc.root_area, "node_visits": tc.node_visits, "leaf_visits": tc.leaf_visits, "tri_tests": tc.tri_tests}


def measure(args):
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    out = {"what": "art_rebuild_device against art_upload_scene of the moved mesh; art_get_tree_cost against measured node visits",
           "device": torch.cuda.get_device_name(0), "cases": []}
    rng = np.random.default_rng(5)
    n = args.rays
    o = (rng.random((n, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2]).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    for scene in args.scenes.split(","):
        sd = scenes.synthetic_scene(args.triangles, 4) if scene == "c4" else scenes.structured_scene(args.triangles)
        pos, nrm, idx, _, matid = sd._mesh_arrays[-1]
        p2 = deform(pos)
        moved = art.SceneDesc(meshes=[dict(mode=art.MESH_CLOSEST, pos=p2, nrm=nrm, idx=idx, matid=matid)], **sd._kw)
        case = {"scene": scene, "triangles": int(idx.shape[0]), "vertices": int(pos.shape[0])}
        p2g = torch.from_numpy(p2).cuda()
        be.upload_scene(moved)                                            # warm: code objects, allocator
        be.upload_scene(sd); be.rebuild_torch(p2g); torch.cuda.synchronize()
        ups, upb, rbs, info = [], [], [], []
        for _ in range(7):                                                # alternating, in one process
            t0 = time.perf_counter(); be.upload_scene(moved); ups.append((time.perf_counter() - t0) * 1e3)
            upb.append(be.bvh_info().build_ms)
            want = be.export_bvh()
            be.upload_scene(sd)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); be.rebuild_torch(p2g); torch.cuda.synchronize(); rbs.append((time.perf_counter() - t0) * 1e3)
            ri = be.rebuild_info()
            info.append((ri.gather_ms, ri.build_ms, ri.host_ms))
        got = be.export_bvh()
        case["same_tree"] = bool(np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))
        case["upload_wall_ms"] = statistics.median(ups); case["upload_wall_ms_runs"] = ups
        case["upload_build_ms"] = statistics.median(upb)
        case["rebuild_wall_ms"] = statistics.median(rbs); case["rebuild_wall_ms_runs"] = rbs
        case["rebuild_gather_ms"], case["rebuild_build_ms"], case["rebuild_host_ms"] = (statistics.median(v) for v in zip(*info))
        case["upload_over_rebuild"] = case["upload_wall_ms"] / case["rebuild_wall_ms"]
        be.upload_scene(sd)
        case["uploaded"] = {"cost": cost(be), "visits_per_ray": visits(be, o, d)}
        case["sweep"] = []
        for amount in [float(a) for a in args.amounts.split(",")]:
            pa = torch.from_numpy(deform(pos, amount)).cuda()
            be.upload_scene(sd)
            be.refit_torch(pa, check=False); torch.cuda.synchronize()
            refitted = {"cost": cost(be), "visits_per_ray": visits(be, o, d)}
            be.rebuild_torch(pa)
            rebuilt = {"cost": cost(be), "visits_per_ray": visits(be, o, d)}
            row = {"amount": amount, "refitted": refitted, "rebuilt": rebuilt,
                   "cost_ratio": refitted["cost"]["node_visits"] / rebuilt["cost"]["node_visits"],
                   "visits_ratio": refitted["visits_per_ray"] / rebuilt["visits_per_ray"]}
            print(json.dumps(row), flush=True)
            case["sweep"].append(row)
            del pa
        print(json.dumps({k: v for k, v in case.items() if k != "sweep"}), flush=True)
        out["cases"].append(case)
        del p2g
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "measure.json"), "w") as f:
        json.dump(out, f, indent=1)
    be.shutdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="output directory of measure.json")
    ap.add_argument("--scenes", default="c4,s4")
    ap.add_argument("--amounts", default="0.25,0.5,1,2")
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--rays", type=int, default=1 << 20)
    measure(ap.parse_args())
