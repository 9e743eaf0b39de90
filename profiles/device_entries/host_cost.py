#!/usr/bin/env python3
"""Host cost of two device-resident entries, for comparing two builds of libart_hip.so (the entries' kernels are the same objects, so
only what the host does per call can differ).

    python profiles/device_entries/host_cost.py LIBRARY [LIBRARY ...] [--rounds 3] [--calls 1000] [--out FILE.json]

Each round visits every library in the order given, each visit in a child process of its own (the library is a process-wide
singleton): 1000 art_occluded_rays_device calls of 4096 rays, then 1000 art_temporal_device calls at 41 x 25, wall clock around each
loop with one synchronize at the end, after 100 untimed calls.  Prints and writes microseconds per call for every visit."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, RAYS = 41, 25, 4096


def child(lib_path, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    art.LIB_PATH = lib_path
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    L = be.lib
    be.upload_scene(scenes.synthetic_scene(2000, 3))
    rng = np.random.default_rng(1)
    o = torch.from_numpy((rng.random((RAYS, 3)) * [4.0, 4.0, 4.0] + [-2.0, 0.5, 0.3]).astype(np.float32)).cuda()
    d = rng.normal(size=(RAYS, 3))
    d = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).cuda()
    occ = torch.empty(RAYS, dtype=torch.uint8, device="cuda")
    N = W * H
    z = lambda k: torch.zeros(k * N, dtype=torch.float32, device="cuda")
    color, mom, hist = z(3), z(2), z(12)
    p = art.ArtTemporalParams()
    ident = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]
    p.cur = p.prev = be.temporal_camera(((0.0, 0.0, 0.0), ident), W, H)
    p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = 2, 16, 1.0, 0.05, 0.9
    pp = C.byref(p)
    a = [x.data_ptr() for x in (o, d, occ, color, mom, hist)]

    def occluded():
        return L.art_occluded_rays_device(a[0], a[1], None, None, RAYS, a[2], None)

    def temporal():
        return L.art_temporal_device(pp, a[3], a[4], None, None, None, None, a[5], None, None, None, None)
    res = {}
    for name, call in (("occluded_us", occluded), ("temporal_us", temporal)):
        for _ in range(100):
            assert call() == 0, L.art_last_error().decode()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        res[name] = (time.perf_counter() - t0) / calls * 1e6
    be.shutdown()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libraries", nargs="+")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.libraries[0]), args.calls)
    visits = []
    for r in range(args.rounds):
        for lib in args.libraries:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), lib], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.exit("%s failed (%d):\n%s" % (lib, out.returncode, out.stderr[-2000:]))
            visits.append(dict(json.loads(out.stdout.strip().splitlines()[-1]), library=lib, round=r))
            print(json.dumps(visits[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rays": RAYS, "frame": [W, H], "calls": args.calls, "visits": visits}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
