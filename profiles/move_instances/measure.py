"""Moving the instances of an instanced scene on the MI355X: art_move_instances_device against the art_upload_scene it replaces (the
upload's path is the one of the commit before the move existed: nothing in it changed), and what the kept instance tree costs.

For I64 (scenes.instanced_scene(): 64 instances x 20 k triangles) and I4096 (4096 instances x 300 triangles), default options:
  upload_wall_ms      wall time of art_upload_scene of the moved scene (host trees, host instance tree, copies), median of 5
  move_host_ms        host time of move_instances_torch(m, check=False) (no wait), median of 9; move_wall_ms: the same + torch.cuda.synchronize()
  move_gpu_ms         ArtMoveInfo.move_ms per move (HIP events around device 0's kernels), median over those of the same 9 that re-padded
                      nothing (the pad bound holds |minv_r3|, so even a jitter of the translations can outgrow a pad: one untimed move to
                      the jittered placement comes first, and `move_repads` records what every timed move re-padded)
  move_gpu_repad_ms   the same for a move that shrinks one instance to 1e-3: its mesh's boxes are re-padded (`repads` >= 1, checked)
  plan_ms             ArtMoveInfo.plan_ms of the first move after the upload
  visits              node visits per ray (count_tests, random rays through art_trace_rays) of the moved scene against a fresh upload at the
                      same matrices, after a jitter of the translations (+-0.02) and after a permutation of the translations

usage: python profiles/move_instances/measure.py --out DIR [--scenes i64,i4096] [--rays 262144]
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


def visits(be, o, d):
    _, st = be.trace_rays(o, d, want_stats=True)
    return st.node_visits / max(1, st.traced_rays)


def measure(args):
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    out = {"what": "art_move_instances_device against art_upload_scene of the moved scene; node visits of the kept instance tree",
           "device": torch.cuda.get_device_name(0), "cases": []}
    rng = np.random.default_rng(5)
    n = args.rays
    o = (rng.random((n, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2]).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    for scene in args.scenes.split(","):
        ni, nt = (64, 20000) if scene == "i64" else (4096, 300)
        sd = scenes.instanced_scene(ni, nt)
        m0 = mats(sd)
        mesh = [int(sd.desc.instances[i].mesh) for i in range(ni)]

        def at(m):
            return scenes.instanced_scene(0, nt, transforms=[(mesh[i], m[i]) for i in range(ni)])
        jit = m0.copy(); jit[:, :, 3] += rng.uniform(-0.02, 0.02, (ni, 3)).astype(np.float32)
        perm = m0.copy(); perm[:, :, 3] = m0[rng.permutation(ni), :, 3]
        tiny = jit.copy(); tiny[0, :, :3] *= np.float32(1.0e-3 / 0.4)
        case = {"scene": scene, "instances": ni, "triangles_per_mesh": nt}
        moved = at(jit)
        be.upload_scene(moved)                                            # warm
        ups = []
        for _ in range(5):
            t0 = time.perf_counter(); be.upload_scene(moved); ups.append((time.perf_counter() - t0) * 1e3)
        case["upload_wall_ms"] = statistics.median(ups); case["upload_wall_ms_runs"] = ups
        be.upload_scene(sd)
        g = {k: torch.from_numpy(v.copy()).cuda() for k, v in (("m0", m0), ("jit", jit), ("perm", perm), ("tiny", tiny))}
        be.move_instances_torch(g["m0"], check=False); torch.cuda.synchronize()
        mi = be.move_info()
        case["plan_ms"] = mi.plan_ms
        be.move_instances_torch(g["jit"], check=False); torch.cuda.synchronize()      # untimed: the pads grow to what the jittered placement asks
        host, wall, gpu, rep = [], [], [], []
        for k in range(9):
            before = be.move_info()
            torch.cuda.synchronize()
            t0 = time.perf_counter(); be.move_instances_torch(g["jit" if k % 2 == 0 else "m0"], check=False); t1 = time.perf_counter()
            torch.cuda.synchronize(); t2 = time.perf_counter()
            after = be.move_info()
            host.append((t1 - t0) * 1e3); wall.append((t2 - t0) * 1e3); gpu.append(after.move_ms - before.move_ms); rep.append(int(after.repads - before.repads))
        plain = [k for k in range(9) if rep[k] == 0]
        if not plain:
            raise SystemExit("every timed move re-padded a mesh: no figure for a move without a re-pad")
        case["move_repads"] = rep
        case["move_host_ms"] = statistics.median(host[k] for k in plain); case["move_wall_ms"] = statistics.median(wall[k] for k in plain)
        case["move_gpu_ms"] = statistics.median(gpu[k] for k in plain)
        before = be.move_info()
        be.move_instances_torch(g["tiny"], check=False)
        after = be.move_info()
        case["move_gpu_repad_ms"] = after.move_ms - before.move_ms; case["repads"] = int(after.repads - before.repads)
        if case["repads"] < 1:
            raise SystemExit("the shrink to 1e-3 re-padded nothing")
        case["upload_over_move_wall"] = case["upload_wall_ms"] / case["move_wall_ms"]
        case["visits"] = {}
        for name, m in (("jitter", jit), ("permutation", perm)):
            be.upload_scene(at(m))
            fresh = visits(be, o, d)
            be.upload_scene(sd)
            be.move_instances_torch(g["jit" if name == "jitter" else "perm"], check=False)
            got = visits(be, o, d)
            case["visits"][name] = {"fresh_upload": fresh, "moved": got, "ratio": got / fresh}
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        del g
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "measure.json"), "w") as f:
        json.dump(out, f, indent=1)
    be.shutdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="output directory of measure.json")
    ap.add_argument("--scenes", default="i64,i4096")
    ap.add_argument("--rays", type=int, default=1 << 18)
    measure(ap.parse_args())
