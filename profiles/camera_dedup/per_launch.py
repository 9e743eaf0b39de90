"""Per-launch times of the trace kernel by its position in a batch, from a `rocprofv3 --kernel-trace --output-format csv` run of bench.py.
A batch of the record schedule at depth D launches the trace kernel D + 1 times: position 0 walks the camera rays, position b the rays
bounce b - 1 emitted.  A batch starts at its k_raygen launch; trace launches before the first one, or beyond depth + 1 in a batch, are left out.
    python profiles/camera_dedup/per_launch.py <..._kernel_trace.csv> [--depth 8]
Prints a markdown table: mean ms per position, its share of the trace kernel's and of all kernels' time."""
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
    per = args.depth + 1
    pos_ms = collections.defaultdict(list)
    by_kernel = collections.defaultdict(float)
    k, pos = 0, None          # pos: position of the next trace launch in its batch; None until the first k_raygen (a launch outside a batch is not counted)
    for r in rows:
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        name = r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("art::", "")
        by_kernel[name] += ms
        if name.endswith("k_raygen"):
            pos = 0           # a batch starts: positions are keyed off its raygen launch, not off a running count
        elif name.endswith("k_trace_coop") and pos is not None and pos < per:
            pos_ms[pos].append(ms)
            pos += 1
            k += 1
    total = sum(by_kernel.values())
    trace = sum(sum(v) for v in pos_ms.values())
    print("trace launches in batches: %d (%d batches), trace %.1f ms of %.1f ms of kernel time\n" % (k, k // per, trace, total))
    print("| position in the batch | launches | mean ms | share of trace | share of all kernel time |")
    print("|---|---|---|---|---|")
    for p in range(per):
        v = pos_ms.get(p, [])
        s = sum(v)
        print("| %d | %d | %.2f | %.1f %% | %.1f %% |" % (p, len(v), s / max(1, len(v)), 100.0 * s / max(trace, 1e-9), 100.0 * s / max(total, 1e-9)))
    print("\n| kernel | ms | share |\n|---|---|---|")
    for name, ms in sorted(by_kernel.items(), key=lambda kv: -kv[1])[:8]:
        print("| `%s` | %.1f | %.2f %% |" % (name, ms, 100.0 * ms / total))


if __name__ == "__main__":
    main()
