"""Device-resident ray queries against the host path, on the MI355X.

For scenes C4 (1 M random triangles) and S4 (1 M structured triangles) and 1 M / 16 M / 64 M random rays:
  host_s      wall time of art_trace_rays on host arrays (AoS -> SoA loop, copies, trace, copies, surface_at loop)
  device_s    wall time of Backend.trace_rays_torch on GPU tensors, including the torch.cuda.synchronize() that ends it
  same_bytes  the 44-byte records of both paths are equal
and, for shadow rays (surface points of the random rays towards samples next to the sphere lights, tnear 1e-4, tfar 0.999 x distance):
  shadow_closest_s / shadow_occluded_s   trace_rays_torch / occluded_torch, same rays and intervals, synchronised.
Device times are the median of 3 runs after one warm-up run; the host path runs once per case.  Kernel times (k_query_pack,
k_analytic, the trace kernel, k_query_finalize, k_query_occluded) come from a separate `rocprofv3 --kernel-trace --stats` run of this
script with --device-only; --rocpd folds that run's database into the JSON (kernel_ms per case).

usage: python profiles/ray_queries/measure.py --out DIR [--device-only] [--rays 1,16,64] [--scenes c4,s4]
       rocprofv3 --kernel-trace --stats -d DIR/rocprof -o run -- python profiles/ray_queries/measure.py --out DIR --device-only
       python profiles/ray_queries/measure.py --rocpd DIR/rocprof/run_results.db --json DIR/measure.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def rays(torch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    o = torch.rand((n, 3), generator=g, device="cuda") * torch.tensor([4.6, 4.4, 4.6], device="cuda") + torch.tensor([-2.3, 0.3, 0.2], device="cuda")
    d = torch.randn((n, 3), generator=g, device="cuda")
    return o.contiguous(), (d / d.norm(dim=1, keepdim=True)).contiguous()


def shadow_rays(torch, be, sd, o, d, seed):
    h = be.trace_rays_torch(o, d)
    keep = h.is_hit != 0
    p = (o + h.t[:, None] * d)[keep]
    L = sd.desc.lights
    centres = torch.tensor([list(L[i].center) for i in range(sd.desc.n_lights)], device="cuda")
    radius = torch.tensor([L[i].radius for i in range(sd.desc.n_lights)], device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = torch.randint(0, sd.desc.n_lights, (p.shape[0],), generator=g, device="cuda")
    u = torch.randn(p.shape, generator=g, device="cuda")
    s = centres[k] + u / u.norm(dim=1, keepdim=True) * (1.5 * radius[k])[:, None]
    v = s - p
    dist = v.norm(dim=1)
    return p.contiguous(), (v / dist[:, None]).contiguous(), torch.full_like(dist, 1e-4), (dist * 0.999).contiguous()


def timed(torch, fn, reps=3):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def measure(args):
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    be = art.Backend(0)
    out = {"what": "device-resident ray queries vs art_trace_rays (host arrays)", "device": torch.cuda.get_device_name(0), "cases": []}
    for scene in args.scenes.split(","):
        sd = scenes.synthetic_scene(1000000, 4) if scene == "c4" else scenes.structured_scene(1000000)
        be.upload_scene(sd)
        for m in [int(x) for x in args.rays.split(",")]:
            n = m << 20
            o, d = rays(torch, n, 1234 + m)
            case = {"scene": scene, "rays": n}
            case["device_s"], case["device_runs_s"] = timed(torch, lambda: be.trace_rays_torch(o, d))
            if not args.device_only:
                on, dn = o.cpu().numpy(), d.cpu().numpy()
                host = np.empty((n, 11), np.int32)
                t0 = time.perf_counter()
                rc = be.lib.art_trace_rays(on.ctypes.data_as(art.f32p), dn.ctypes.data_as(art.f32p), None, n, host.ctypes.data_as(C.POINTER(art.ArtHit)), art.TRACE_COOP, None)
                case["host_s"] = time.perf_counter() - t0
                assert rc == 0, be.lib.art_last_error().decode()
                dev = be.trace_rays_torch(o, d).raw.cpu().numpy()
                case["same_bytes"] = bool(np.array_equal(dev, host))
                case["host_over_device"] = case["host_s"] / case["device_s"]
                del on, dn, host, dev
            so, sdir, stn, stf = shadow_rays(torch, be, sd, o, d, 99 + m)
            case["shadow_rays"] = int(so.shape[0])
            case["shadow_closest_s"], _ = timed(torch, lambda: be.trace_rays_torch(so, sdir, stn, stf))
            case["shadow_occluded_s"], _ = timed(torch, lambda: be.occluded_torch(so, sdir, stn, stf))
            occ = be.occluded_torch(so, sdir, stn, stf)
            hit = be.trace_rays_torch(so, sdir, stn, stf).is_hit != 0
            case["shadow_occluded_fraction"] = float(occ.float().mean().item())
            case["shadow_occlusion_equals_is_hit"] = bool(torch.equal(occ, hit))
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            del o, d, so, sdir, stn, stf, occ, hit
            torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "measure_device_only.json" if args.device_only else "measure.json"), "w") as f:
        json.dump(out, f, indent=1)
    be.shutdown()


# the queries measure() issues per case, in order: (label or None for an untimed call, kind, ray count key)
CALLS = [(None, "closest", "rays")] + [("random_closest", "closest", "rays")] * 3 + [(None, "closest", "rays")] + \
        [(None, "closest", "shadow_rays")] + [("shadow_closest", "closest", "shadow_rays")] * 3 + \
        [(None, "occluded", "shadow_rays")] + [("shadow_occluded", "occluded", "shadow_rays")] * 3 + [(None, "occluded", "shadow_rays"), (None, "closest", "shadow_rays")]


def fold_rocpd(args):
    """The rocprofv3 database of the --device-only run -> per case and timed query kind, the median kernel time (ms) of every stage of
    one query: k_query_pack, k_analytic, the trace kernel(s), k_query_finalize / k_query_occluded (summed over the query's slices).
    A slice is the dispatches from one k_query_pack to the next finalize / occluded kernel; the slices are matched to the calls of
    measure() in order (CALLS), a call taking slices until their pack grids (rays rounded up to 256) cover its ray count."""
    import sqlite3
    db = sqlite3.connect(args.rocpd)
    rows = db.execute("select name, grid_x, duration from kernels order by start").fetchall()
    stage_of = lambda name: next((k for k in ("k_query_pack", "k_analytic", "k_trace_coop", "k_trace_simple", "k_trace_overflow", "k_count_live",
                                              "k_query_finalize", "k_query_occluded") if k in name), None)
    slices, cur = [], None
    for name, grid, ns in rows:
        st = stage_of(name)
        if st == "k_query_pack":
            cur = {"n256": int(grid), "ms": {}}
        if cur is None or st is None:
            continue
        key = "trace" if st.startswith("k_trace") else st
        cur["ms"][key] = cur["ms"].get(key, 0.0) + ns / 1e6
        if st in ("k_query_finalize", "k_query_occluded"):
            cur["kind"] = "closest" if st == "k_query_finalize" else "occluded"
            slices.append(cur); cur = None
    data = json.load(open(args.json))
    k = 0
    for case in data["cases"]:
        timed_q = {}
        for label, kind, nkey in CALLS:
            q, covered = {}, 0
            while covered < case[nkey]:
                sl = slices[k]; k += 1
                assert sl["kind"] == kind, "slice %d: %s, expected %s" % (k - 1, sl["kind"], kind)
                covered += sl["n256"]
                for st, ms in sl["ms"].items():
                    q[st] = q.get(st, 0.0) + ms
            if label:
                timed_q.setdefault(label, []).append(q)
        case["kernel_ms"] = {}
        for label, qs in timed_q.items():
            med = {st: statistics.median([q.get(st, 0.0) for q in qs]) for st in sorted({st for q in qs for st in q})}
            med["total"] = statistics.median([sum(q.values()) for q in qs])
            tr = med.get("k_analytic", 0.0) + med.get("trace", 0.0)
            med["pack_plus_finalize_over_analytic_plus_trace"] = (med.get("k_query_pack", 0.0) + med.get("k_query_finalize", 0.0) + med.get("k_query_occluded", 0.0)) / tr
            case["kernel_ms"][label] = med
    assert k == len(slices), "%d slices left over" % (len(slices) - k)
    with open(args.json, "w") as f:
        json.dump(data, f, indent=1)
    for c in data["cases"]:
        print(c["scene"], c["rays"], json.dumps({l: {s: round(v, 3) for s, v in m.items()} for l, m in c["kernel_ms"].items()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="output directory of measure.json")
    ap.add_argument("--rays", default="1,16,64", help="ray counts in units of 2^20")
    ap.add_argument("--scenes", default="c4,s4")
    ap.add_argument("--device-only", action="store_true", help="skip the host path (the profiler run)")
    ap.add_argument("--rocpd", default=None, help="rocprofv3 database of a --device-only run: fold its kernel times into --json")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not a.rocpd and not a.out:
        ap.error("--out is required")
    fold_rocpd(a) if a.rocpd else measure(a)
