"""Deforming a mesh of an instanced scene on the MI355X: art_refit_mesh_device against the art_upload_scene it replaces (the upload's
path is the one of the commit before the call existed: nothing in it changed), and what the kept trees cost.

For I64 (scenes.instanced_scene(): 64 instances of two 20 k-triangle meshes), default options, mesh 0 (the torus) deformed:
  upload_wall_ms      wall time of art_upload_scene of the deformed scene (host trees, host instance tree, copies), median of 5
  refit_host_ms       host time of refit_mesh_torch(0, pos, nrm, check=False) (no wait), median of 9; refit_wall_ms: the same +
                      torch.cuda.synchronize()
  refit_gpu_ms        ArtMeshRefitInfo.refit_ms per refit (HIP events around device 0's kernels: records, the mesh's tree level by level,
                      pads, entry-point boxes, instance tree), median of the same 9, which alternate between the deformed and the uploaded
                      vertices; `refit_repads` records what every timed refit re-padded
  plan_ms             ArtMeshRefitInfo.plan_ms of the first refit after the upload
  visits              node visits per ray (count_tests, random rays through art_trace_rays) of the refitted scene against a fresh upload
                      of the same deformed scene, after a moderate deformation (a twist of 0.6 rad per unit of y, y stretched by 1.3)

usage: python profiles/refit_instanced/measure.py --out DIR [--rays 262144]
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


def twisted(pos, nrm, sy, k):
    a = k * pos[:, 1].astype(np.float64)
    c, s = np.cos(a), np.sin(a)

    def rot(v):
        v = v.astype(np.float64)
        return np.stack([c * v[:, 0] + s * v[:, 2], v[:, 1], -s * v[:, 0] + c * v[:, 2]], 1)
    p = rot(pos); p[:, 1] *= sy
    n = rot(nrm); n[:, 1] /= sy; n /= np.linalg.norm(n, axis=1, keepdims=True)
    return p.astype(np.float32), n.astype(np.float32)


def visits(be, o, d):
    _, st = be.trace_rays(o, d, want_stats=True)
    return st.node_visits / max(1, st.traced_rays)


def measure(args):
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    out = {"what": "art_refit_mesh_device against art_upload_scene of the deformed scene; node visits of the kept trees",
           "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(5)
    n = args.rays
    o = (rng.random((n, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2]).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    sd = scenes.instanced_scene()
    arrays = sd._mesh_arrays
    p0, n0 = arrays[0][0].copy(), arrays[0][1].copy()
    p1, n1 = twisted(p0, n0, 1.3, 0.6)
    ms = [dict(mode=art.MESH_CLOSEST, pos=p1 if k == 0 else a[0], nrm=n1 if k == 0 else a[1], idx=a[2], uv=a[3], matid=a[4]) for k, a in enumerate(arrays)]
    inst = [(int(sd.desc.instances[i].mesh), list(sd.desc.instances[i].m)) for i in range(sd.desc.n_instances)]
    deformed = art.SceneDesc(meshes=ms, instances=inst, **sd._kw)
    case = {"scene": "i64", "instances": sd.desc.n_instances, "mesh": 0, "vertices": int(p0.shape[0]), "triangles": int(arrays[0][2].shape[0])}
    be.upload_scene(deformed)                                             # warm
    ups = []
    for _ in range(5):
        t0 = time.perf_counter(); be.upload_scene(deformed); ups.append((time.perf_counter() - t0) * 1e3)
    case["upload_wall_ms"] = statistics.median(ups); case["upload_wall_ms_runs"] = ups
    fresh = visits(be, o, d)
    be.upload_scene(sd)
    g = [(torch.from_numpy(p1).cuda(), torch.from_numpy(n1).cuda()), (torch.from_numpy(p0).cuda(), torch.from_numpy(n0).cuda())]
    be.refit_mesh_torch(0, g[1][0], g[1][1], check=False); torch.cuda.synchronize()
    case["plan_ms"] = be.mesh_refit_info().plan_ms
    host, wall, gpu, rep = [], [], [], []
    for k in range(9):
        before = be.mesh_refit_info()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); be.refit_mesh_torch(0, g[k % 2][0], g[k % 2][1], check=False); t1 = time.perf_counter()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        after = be.mesh_refit_info()
        host.append((t1 - t0) * 1e3); wall.append((t2 - t0) * 1e3); gpu.append(after.refit_ms - before.refit_ms); rep.append(int(after.repads - before.repads))
    case["refit_repads"] = rep
    case["refit_host_ms"] = statistics.median(host); case["refit_wall_ms"] = statistics.median(wall); case["refit_gpu_ms"] = statistics.median(gpu)
    case["upload_over_refit_wall"] = case["upload_wall_ms"] / case["refit_wall_ms"]
    got = visits(be, o, d)                                                # (the ninth refit left the deformed vertices)
    case["visits"] = {"fresh_upload": fresh, "refitted": got, "ratio": got / fresh}
    print(json.dumps(case), flush=True)
    out["cases"] = [case]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "measure.json"), "w") as f:
        json.dump(out, f, indent=1)
    be.shutdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="output directory of measure.json")
    ap.add_argument("--rays", type=int, default=1 << 18)
    measure(ap.parse_args())
