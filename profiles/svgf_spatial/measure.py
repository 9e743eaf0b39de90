"""GPU time of art_svgf_spatial_variance_device, measured once on one MI355X at 1920 x 1080.

One process, the calls alternating round by round (so drift and other tenants hit all of them alike), each timed by device events around
INNER back-to-back calls on the library's stream:
  spatial_short_r1 / _r2 / _r3   the first-frame case: every pixel has one colour and a variance of +infinity, so every lane runs the window
  spatial_long                   steady state: every pixel has 8 colours and a finite variance, so every wave leaves after the copy
  temporal                       art_temporal_device, cameras at rest, every plane given, history in and out
  svgf_var_1_iteration           art_denoise_svgf_var_device with iterations = 1 (its pack kernel, one filter launch, the finish)
against the byte floors at the 6.3 TB/s profiles/denoise/ measured: 8 B per pixel for the copy (the variance word in and out), and for
the short case each record of the three history planes once plus the same 8 B: 56 B per pixel.  Neither floor counts the n word of a
long pixel, which lies at a stride of 16 bytes: its plane travels whole (16 B per pixel more).

The history is synthetic (a slanted floor with a nearer panel over the right third, random moments): the kernel's time depends on the
lengths and on which taps are finite, not on a scene.

usage: python profiles/svgf_spatial/measure.py [--out profiles/svgf_spatial/measure.json] [--reps 10] [--inner 20]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
BANDWIDTH_TBS = 6.3          # profiles/denoise/README.md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf_spatial", "measure.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    art = ge.load_package()
    be = art.Backend(0)
    N = W * H
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    X = torch.arange(W, device="cuda", dtype=torch.float32).expand(H, W)
    Y = torch.arange(H, device="cuda", dtype=torch.float32).unsqueeze(1).expand(H, W)
    pan = X >= (2 * W) // 3
    z = 10.0 + 0.005 * X + 0.002 * Y - 4.0 * pan
    lum = 0.2 + 1.8 * torch.rand((H, W), device="cuda", generator=gen)

    def history(n):
        h = torch.zeros((3, H, W, 4), device="cuda")
        h[0, ..., :3] = lum.unsqueeze(-1); h[0, ..., 3] = n
        h[1, ..., 0] = lum; h[1, ..., 1] = lum * lum * (1.0 + torch.rand((H, W), device="cuda", generator=gen)); h[1, ..., 2] = z
        h[2, ..., 0] = 0.6 * pan; h[2, ..., 2] = torch.where(pan, 0.8, 1.0)
        return h.contiguous()
    h_short, h_long = history(1.0), history(8.0)
    v_short = torch.full((H, W), float("inf"), device="cuda")
    v_long = (h_long[1, ..., 1] - h_long[1, ..., 0] ** 2).clamp(min=0) / 7.0
    out = torch.empty((H, W), device="cuda")
    # the neighbours: a frame for art_temporal_device (cameras at rest) and the variance-plane filter
    eye = np.eye(4, dtype=np.float32)
    cam = (np.zeros(3, np.float32), eye)
    cur = dict(color=lum.unsqueeze(-1).repeat(1, 1, 3).contiguous(), moments=torch.stack([lum, lum * lum], -1).contiguous(),
               normal=h_long[2, ..., :3].contiguous(), depth=z.contiguous(), prim_index=torch.ones((H, W), dtype=torch.int32, device="cuda"))
    albedo = torch.full((H, W, 3), 0.5, device="cuda")
    fout = torch.empty((H, W, 3), device="cuda")
    calls = {
        "spatial_short_r1": lambda: be.svgf_spatial_variance_torch(h_short, v_short, W, H, radius=1, min_history=4.0, sigma_depth=1.0, out=out),
        "spatial_short_r2": lambda: be.svgf_spatial_variance_torch(h_short, v_short, W, H, radius=2, min_history=4.0, sigma_depth=1.0, out=out),
        "spatial_short_r3": lambda: be.svgf_spatial_variance_torch(h_short, v_short, W, H, radius=3, min_history=4.0, sigma_depth=1.0, out=out),
        "spatial_long": lambda: be.svgf_spatial_variance_torch(h_long, v_long, W, H, radius=3, min_history=4.0, sigma_depth=1.0, out=out),
        "temporal": lambda: be.temporal_torch(cur, h_long, cam, cam, 1),
        "svgf_var_1_iteration": lambda: be.denoise_svgf_torch(cur["color"], variance=v_long, albedo=albedo, normal=cur["normal"], depth=cur["depth"],
                                                              iterations=1, out=fout),
    }
    # the shipped defaults too (radius, min_history and sigma_depth of the package) on the first-frame case
    calls["spatial_short_defaults"] = lambda: be.svgf_spatial_variance_torch(h_short, v_short, W, H, out=out)
    ms = {k: [] for k in calls}
    for r in range(args.reps + 3):                                  # three warm rounds: code objects, torch's allocator
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record(); e1.synchronize()
            if r >= 3:
                ms[name].append(e0.elapsed_time(e1) / args.inner)
    # what the timed calls computed, so that a wrong run is seen: the short case finds a variance, the long case is the copy
    be.svgf_spatial_variance_torch(h_short, v_short, W, H, radius=3, min_history=4.0, sigma_depth=1.0, out=out)
    finite_share = float(torch.isfinite(out).float().mean())
    be.svgf_spatial_variance_torch(h_long, v_long, W, H, radius=3, min_history=4.0, sigma_depth=1.0, out=out)
    copy_ok = bool(torch.equal(out, v_long))
    floor = lambda nbytes: nbytes / (BANDWIDTH_TBS * 1e12) * 1e3
    res = {"what": "%d x %d, one MI355X; per call, the mean over %d back-to-back calls between two device events; %d rounds after 3 warm ones, "
                   "the calls alternating inside every round" % (W, H, args.inner, args.reps),
           "ms": {k: {"mean": statistics.mean(v), "stdev": statistics.pstdev(v), "min": min(v)} for k, v in ms.items()},
           "floor_ms": {"copy_8B_per_pixel": floor(8 * N), "short_56B_per_pixel": floor(56 * N), "long_with_plane0_24B_per_pixel": floor(24 * N)},
           "defaults": {"radius": art.SVGF_SPATIAL_RADIUS, "min_history": art.SVGF_SPATIAL_MIN_HISTORY, "sigma_depth": art.SVGF_SPATIAL_SIGMA_DEPTH},
           "short_case_finite_share": finite_share, "long_case_is_the_copy": copy_ok,
           "lds_variant": "not attempted: the direct-load kernel is the only one"}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    be.shutdown()


if __name__ == "__main__":
    main()
