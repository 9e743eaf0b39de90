"""GPU time of art_auto_exposure_device and art_display_device, measured once on one MI355X at 1920 x 1080.

One process, the calls alternating round by round (so drift and other tenants hit all of them alike), each timed by device events around
INNER back-to-back calls on the library's stream:
  exposure_spread       the histogram and the walk over an HDR frame whose luminances spread over about 200 bins
  exposure_one_bin      every pixel in ONE bin: all 256 lanes of a workgroup add to one LDS counter (the contention case)
  exposure_black        every pixel black: bin 0 without a log_pos, the same contention -- exposure_one_bin minus this is the binary64
                        log_pos; exposure_one_bin minus exposure_spread is the contention
  display_aces_srgb     ACES, the sRGB transfer (one binary64 apow per channel above the linear toe), dither, screen words only
  display_aces_srgb_ldr the same with the ldr plane too (16 B written per pixel instead of 4)
  display_aces_sqrt     ACES, sqrtf, dither: display_aces_srgb minus this is the three apow
  display_reference     ART_CURVE_REFERENCE (resolve_pixel)
  display_xmajor        display_aces_srgb in ART_LAYOUT_ADA_XY (stores strided by the height)
  denoise_1_iteration   art_denoise_device with iterations = 1 on the same frame, the yardstick of the other READMEs
against the compulsory bytes at the 6.3 TB/s profiles/denoise/ measured: 12 B per pixel read for the histogram; 12 B read and 4 B (screen)
or 16 B (screen and ldr) written for the display.

What a figure is: the time between two device events around INNER calls issued from Python, divided by INNER.  Where a call's kernels
are shorter than the host takes to issue the next call (tens of microseconds: the display calls, perhaps all of them), the queue runs
empty and the figure is the host's issue rate, not kernel time: every figure is an UPPER BOUND of the GPU time per call, and differences
of a few microseconds between two of them (the log_pos, the x-major stores) are not resolved.  `host_issue_ms` is the host's own time per
call of each kind (wall clock around the same INNER calls, without waiting), to hold against the figure beside it.

profiles/display/measure_2048_workgroups.json is this script's output from the one run with kExpBlocks = 2048 in csrc/art_display.hip
(8 workgroups per CU) instead of the 512 that are kept; it is a file of its own so that a new run does not overwrite it.

usage: python profiles/display/measure.py [--out profiles/display/measure.json] [--reps 10] [--inner 20]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
BANDWIDTH_TBS = 6.3          # profiles/denoise/README.md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display", "measure.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import __graft_entry__ as ge
    art = ge.load_package()
    be = art.Backend(0)
    N = W * H
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    spread = torch.exp(torch.empty((H, W, 3), device="cuda").uniform_(-6.9, 3.9, generator=gen)).contiguous()      # 1e-3 .. 50 per channel
    one_bin = torch.tensor([0.25, 0.3, 0.2], device="cuda").expand(H, W, 3).contiguous()
    black = torch.zeros((H, W, 3), device="cuda")
    state = be.exposure_state()
    screen = torch.empty((H, W), dtype=torch.int32, device="cuda")
    screen_x = torch.empty((W, H), dtype=torch.int32, device="cuda")
    albedo = torch.full((H, W, 3), 0.5, device="cuda")
    normal = torch.zeros((H, W, 3), device="cuda"); normal[..., 2] = 1.0
    depth = (10.0 + 0.005 * torch.arange(W, device="cuda", dtype=torch.float32)).expand(H, W).contiguous()
    fout = torch.empty((H, W, 3), device="cuda")
    kw = dict(curve=art.display.CURVE_ACES, transfer=art.display.TRANSFER_SRGB, dither=True)
    calls = {
        "exposure_spread": lambda: be.auto_exposure_torch(spread, state, adapt=0.5),
        "exposure_one_bin": lambda: be.auto_exposure_torch(one_bin, state, adapt=0.5),
        "exposure_black": lambda: be.auto_exposure_torch(black, state, adapt=0.5),
        "display_aces_srgb": lambda: be.display_torch(spread, state, out=screen, **kw),
        "display_aces_srgb_ldr": lambda: be.display_torch(spread, state, out=screen, want_ldr=True, **kw),
        "display_aces_sqrt": lambda: be.display_torch(spread, state, out=screen, **dict(kw, transfer=art.display.TRANSFER_SQRT)),
        "display_reference": lambda: be.display_torch(spread, out=screen, curve=art.display.CURVE_REFERENCE),
        "display_xmajor": lambda: be.display_torch(spread, state, out=screen_x, layout=art.LAYOUT_ADA_XY, **kw),
        "denoise_1_iteration": lambda: be.denoise_torch(spread, albedo=albedo, normal=normal, depth=depth, iterations=1, out=fout),
    }
    ms = {k: [] for k in calls}
    host = {k: [] for k in calls}
    for r in range(args.reps + 3):                                  # three warm rounds: code objects, torch's allocator
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            t1 = time.perf_counter()
            e1.record(); e1.synchronize()
            if r >= 3:
                ms[name].append(e0.elapsed_time(e1) / args.inner)
                host[name].append((t1 - t0) * 1e3 / args.inner)
    # what the timed calls computed, so that a wrong run is seen
    fresh = be.exposure_state()
    be.auto_exposure_torch(spread, fresh)
    torch.cuda.synchronize()
    words = fresh.cpu()
    bins_used = int((words[5:259] != 0).sum())
    counted = int(words[2])
    be.auto_exposure_torch(one_bin, fresh)
    one_bin_bins = int((fresh.cpu()[4:] != 0).sum())
    be.display_torch(spread, state, out=screen, **kw)
    distinct = int(torch.unique(screen).numel())
    floor = lambda nbytes: nbytes / (BANDWIDTH_TBS * 1e12) * 1e3
    stat = {k: {"mean": statistics.mean(v), "stdev": statistics.pstdev(v), "min": min(v)} for k, v in ms.items()}
    floors = {"exposure_12B_per_pixel": floor(12 * N), "display_16B_per_pixel": floor(16 * N), "display_with_ldr_28B_per_pixel": floor(28 * N)}
    dn = stat["denoise_1_iteration"]["mean"]
    res = {"what": "%d x %d, one MI355X; per call, the mean over %d back-to-back calls between two device events; %d rounds after 3 warm ones, "
                   "the calls alternating inside every round" % (W, H, args.inner, args.reps),
           "caveat": "every ms figure is an upper bound of the GPU time per call: where the host issues calls more slowly than the kernels run, "
                     "it is the host's issue rate (host_issue_ms beside it); differences of a few microseconds are not resolved",
           "ms": stat, "host_issue_ms": {k: statistics.mean(v) for k, v in host.items()}, "floor_ms": floors,
           "ratio_to_denoise_1_iteration": {k: v["mean"] / dn for k, v in stat.items()},
           "ratio_to_floor": {"exposure_spread": stat["exposure_spread"]["mean"] / floors["exposure_12B_per_pixel"],
                              "exposure_one_bin": stat["exposure_one_bin"]["mean"] / floors["exposure_12B_per_pixel"],
                              "exposure_black": stat["exposure_black"]["mean"] / floors["exposure_12B_per_pixel"],
                              "display_aces_srgb": stat["display_aces_srgb"]["mean"] / floors["display_16B_per_pixel"],
                              "display_aces_sqrt": stat["display_aces_sqrt"]["mean"] / floors["display_16B_per_pixel"],
                              "display_reference": stat["display_reference"]["mean"] / floors["display_16B_per_pixel"],
                              "display_xmajor": stat["display_xmajor"]["mean"] / floors["display_16B_per_pixel"],
                              "display_aces_srgb_ldr": stat["display_aces_srgb_ldr"]["mean"] / floors["display_with_ldr_28B_per_pixel"]},
           "binary64_log_pos_ms": stat["exposure_one_bin"]["mean"] - stat["exposure_black"]["mean"],
           "lds_contention_ms": stat["exposure_one_bin"]["mean"] - stat["exposure_spread"]["mean"],
           "three_apow_ms": stat["display_aces_srgb"]["mean"] - stat["display_aces_sqrt"]["mean"],
           "spread_frame": {"bins_used": bins_used, "counted": counted}, "one_bin_frame_bins": one_bin_bins, "distinct_screen_words": distinct,
           "wave_level_pre_aggregation": "not attempted: one LDS add per lane is the only variant"}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    be.shutdown()


if __name__ == "__main__":
    main()
