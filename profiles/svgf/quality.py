"""Which defaults Backend.denoise_svgf_torch ships: a sweep of sigma_color x iterations on the CPU, before any GPU run.

Scene and frame: scenes.synthetic_scene(2000, 3) at 48 x 48, PT_MIS, depth 8 (the frame behind the README's RMS figure of the plain
filter).  The noisy frames are the CPU oracle's per-sample radiance at 4, 8 and 16 spp (seed 7), WITHOUT anti-aliasing: with it a colour
is a group of four samples, so 4 spp would be one colour per pixel and no variance (n_colours >= 2).  The reference picture is the
oracle's 1024 spp of the same estimator (seed 11).  The feature buffers are the first hits of the pixel centres through the product's
host build (tests/hostsim.py), in the arithmetic of include/art_hip.h.  The filters are the numpy references (tests/svgf_ref.py,
tests/denoise_ref.py), which the kernels equal bit for bit.  RMS over all pixels and channels of (picture - reference).

usage: python profiles/svgf/quality.py [--out profiles/svgf/quality.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32
W = H = 48
SPPS = (4, 8, 16)
SIGMAS = (0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
ITERATIONS = (1, 2, 3, 4, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf", "quality.json"))
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--golden", help="also write the reference picture here (tests/golden/svgf_quality_ref_48x48.npy: the quality tests read it)")
    args = ap.parse_args()
    import __graft_entry__ as ge
    art = ge.load_package()
    from ada_ray_tracer_amd import scenes
    import conv, denoise_ref, hostsim, moments_ref, orc, svgf_ref
    import test_gpu_aov as aov                      # the reference of the feature buffers: camera rays, albedo table, the 4-ray mean
    sd = scenes.synthetic_scene(2000, 3)
    osc = conv.OracleScene(sd)
    nodes, tris, info = hostsim.bvh(art, sd)
    osc.attach_bvh(nodes, tris, info["width"])
    ref, rspp, _ = orc.render(osc.scene, orc.make_params(W, H, orc.PT_MIS, False, 8, 64, seed=11), passes=args.reference_spp // 64)
    ref = ref / F(rspp)
    if args.golden:
        np.save(args.golden, ref.astype(F))
    rad = moments_ref.sample_radiance(osc.scene, orc.make_params(W, H, orc.PT_MIS, False, 8, 1, seed=7), 0, max(SPPS))
    # feature buffers of the pixel centres
    d = aov.camera_dirs(sd.desc, W, H, False)
    o = np.tile(np.array(list(sd.desc.cam_pos), F), (W * H, 1))
    raw = aov.host_raw(hostsim.trace(art, sd, o, np.ascontiguousarray(d.reshape(-1, 3)))[0]).reshape(W * H, 11)
    f, hit = raw.view(F), raw[:, 1] == 1
    table, _ = aov.albedo_table(art, sd.desc)
    guides = dict(albedo=np.where(hit[:, None], table[np.where(hit, raw[:, 5], 0)], F(0)).astype(F).reshape(H, W, 3),
                  normal=np.where(hit[:, None], f[:, 6:9], F(0)).astype(F).reshape(H, W, 3), depth=np.where(hit, f[:, 0], F(0)).astype(F).reshape(H, W))
    rms = lambda x: float(np.sqrt(((x.astype(np.float64) - ref) ** 2).mean()))
    rows = []
    frames = {}
    for spp in SPPS:
        acc, mom = moments_ref.add_colours(moments_ref.colours(rad[:spp], False))
        frames[spp] = (acc, mom, rms(acc / F(spp)))
    for sc in SIGMAS:
        for it in ITERATIONS:
            row = {"sigma_color": sc, "iterations": it, "spp": {}}
            for spp in SPPS:
                acc, mom, before = frames[spp]
                plain = denoise_ref.denoise(acc, **guides, iterations=it, scale=1.0 / spp, sigma_color=sc)
                svgf, _ = svgf_ref.denoise(acc, mom, spp, **guides, iterations=it, scale=1.0 / spp, sigma_color=sc)
                row["spp"][str(spp)] = {"input": before, "plain": rms(plain), "svgf": rms(svgf)}
            row["svgf_worst_ratio"] = max(v["svgf"] / v["input"] for v in row["spp"].values())
            row["plain_worst_ratio"] = max(v["plain"] / v["input"] for v in row["spp"].values())
            rows.append(row)
            print("sigma_color %5.1f  iterations %d  " % (sc, it) + "  ".join(
                "%2d spp: in %.4f plain %.4f svgf %.4f" % (s, row["spp"][str(s)]["input"], row["spp"][str(s)]["plain"], row["spp"][str(s)]["svgf"]) for s in SPPS), flush=True)
    best = min(rows, key=lambda r: r["svgf_worst_ratio"])
    best_plain = min(rows, key=lambda r: r["plain_worst_ratio"])
    res = {"what": "RMS error against %d spp of the same estimator; synthetic_scene(2000, 3), %d x %d, PT_MIS, depth 8, no anti-aliasing; CPU oracle samples, "
                   "numpy reference filters (sigma_depth 1, normal_log2 7, demodulation on)" % (rspp, W, H),
           "reference_spp": rspp, "rows": rows,
           "best_svgf": {k: best[k] for k in ("sigma_color", "iterations", "svgf_worst_ratio", "spp")},
           "best_plain": {k: best_plain[k] for k in ("sigma_color", "iterations", "plain_worst_ratio", "spp")},
           "svgf_improves_at_every_spp": best["svgf_worst_ratio"] < 1.0,
           "shipped_defaults": {"sigma_color": art.SVGF_SIGMA_COLOR, "iterations": art.SVGF_ITERATIONS}}
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("best_svgf", "best_plain", "svgf_improves_at_every_spp")}))


if __name__ == "__main__":
    main()
