"""Per-launch times of the trace kernel and of the shade stage by their position in a batch, from a `rocprofv3 --kernel-trace
--output-format csv` run of bench.py (profiles/camera_dedup/per_launch.py with the shade stage next to the trace kernel).
A batch of the record schedule at depth D starts at its k_raygen launch; it launches the trace kernel D + 1 times (position 0: the
camera rays, position b: the records bounce b - 1 emitted) and the shade stage D times (position b: bounce b).
    python profiles/null_shadow/per_launch.py <..._kernel_trace.csv> [--depth 8]
Prints a markdown table: launches, mean ms and (max - min) per position for both kernels, then the kernels' totals."""
import argparse
import collections
import csv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--depth", type=int, default=8)
    args = ap.parse_args()
    rows = list(csv.DictReader(open(args.csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    limit = {"k_trace_coop": args.depth + 1, "k_shade_compact": args.depth}
    pos = None                                  # per kernel: position of its next launch in the batch; None until the first k_raygen
    ms_at = {k: collections.defaultdict(list) for k in limit}
    by_kernel = collections.defaultdict(float)
    for r in rows:
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        name = r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("art::", "")
        by_kernel[name] += ms
        if name.endswith("k_raygen"):
            pos = {k: 0 for k in limit}
        else:
            k = next((k for k in limit if name.endswith(k)), None)
            if k is not None and pos is not None and pos[k] < limit[k]:
                ms_at[k][pos[k]].append(ms)
                pos[k] += 1
    total = sum(by_kernel.values())
    print("| position | `k_trace_coop` launches | mean ms | max - min | `k_shade_compact` launches | mean ms | max - min |")
    print("|---|---|---|---|---|---|---|")
    for p in range(args.depth + 1):
        cells = []
        for k in ("k_trace_coop", "k_shade_compact"):
            v = ms_at[k].get(p, [])
            cells += ["%d" % len(v), "%.2f" % (sum(v) / len(v)) if v else "", "%.2f" % (max(v) - min(v)) if v else ""]
        print("| %d | %s |" % (p, " | ".join(cells)))
    print("\n| kernel | ms | share of kernel time |\n|---|---|---|")
    for name, ms in sorted(by_kernel.items(), key=lambda kv: -kv[1])[:6]:
        print("| `%s` | %.1f | %.2f %% |" % (name, ms, 100.0 * ms / total))


if __name__ == "__main__":
    main()
