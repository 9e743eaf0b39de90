#!/usr/bin/env python3
"""Are the kernels of art_trace.hip, art_stages.hip and art_frame.hip the kernels of the art_kernels.hip they were cut from?

    python3 profiles/kernel_split/compare.py [--parent REV] [--out profiles/kernel_split/kernels.md]
    python3 profiles/kernel_split/compare.py --objects PARENT_BUILD_DIR THIS_BUILD_DIR [--out profiles/kernel_split/objects.md]

First form: the parent's sources (git archive REV, default HEAD~1) and this tree's are compiled for the device only, each unit with the
compile line its own Makefile prints (make -n), to assembly (-S) with -Rpass-analysis=kernel-resource-usage.  For every kernel, by
mangled name, two things are compared for equality: the resource remarks, and the kernel's text -- its instructions from its label to its
end, and its .amdhsa_kernel descriptor block -- after replacing what only says where in its file the kernel stands (the function number
in .LBB<n>_<k> / .Lfunc_end<n> labels, the numbers of .Ltmp labels) and dropping the assembler comments.  A kernel found on one side
only is reported as such.  The script looks for no particular instruction; it exits 1 unless every kernel is the same.

Second form: the sha256 of the build/*.hip.o of the units that exist on both sides, as a table.
"""
import argparse
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = "ada-ray-tracer_amd"
FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
SHORT = ["sgpr", "vgpr", "agpr", "scratch", "occ", "sgpr spill", "vgpr spill", "lds"]


def compile_line(pkg_dir, unit):
    """the Makefile's own compile line of csrc/<unit>, as a list, without its -c / -o"""
    out = subprocess.check_output(["make", "-n", "-B", "-C", pkg_dir, "build/%s.o" % unit], text=True)
    line = [ln for ln in out.splitlines() if "csrc/" + unit in ln and " -c " in ln][0]
    words = shlex.split(line)
    i = words.index("-o")
    del words[i:i + 2]
    words.remove("-c")
    return words


def device_asm(pkg_dir, unit, workdir):
    """(assembly text, {kernel: [remark values]}) of one unit, device side only"""
    asm = os.path.join(workdir, unit + ".s")
    cmd = compile_line(pkg_dir, unit) + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", asm]
    err = subprocess.run(cmd, cwd=pkg_dir, stderr=subprocess.PIPE, text=True, check=True).stderr
    remarks, cur = {}, None
    for ln in err.splitlines():
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]$", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = remarks.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return open(asm).read(), remarks


def kernel_texts(asm):
    """{kernel: normalised text} -- body (label .. .Lfunc_end) and descriptor (.amdhsa_kernel .. .end_amdhsa_kernel)"""
    lines = asm.splitlines()
    kernels = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    texts = {}
    for k in kernels:
        start = next(i for i, ln in enumerate(lines) if ln.split(";", 1)[0].rstrip() == k + ":")
        end = next(i for i in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        d0 = next(i for i, ln in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(k) + r"$", ln))
        d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        tmp = {}
        out = []
        for ln in lines[start:end] + lines[d0:d1 + 1]:
            ln = ln.split(";", 1)[0].rstrip()
            if not ln:
                continue
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
            ln = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % tmp.setdefault(m.group(0), len(tmp)), ln)
            out.append(ln)
        texts[k] = "\n".join(out)
    return texts


def side(pkg_dir, units, workdir):
    res = {}
    for u in units:
        asm, remarks = device_asm(pkg_dir, u, workdir)
        for k, t in kernel_texts(asm).items():
            res[k] = (u, t, [remarks.get(k, {}).get(f, "?") for f in FIELDS])
    return res


def kernels_table(parent_rev, out_path):
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", parent_rev, PKG + "/csrc", PKG + "/Makefile", PKG + "/flags.mk", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", tmp], stdin=ar.stdout)
        assert ar.wait() == 0
        wp, wt = os.path.join(tmp, "asm_parent"), os.path.join(tmp, "asm_this")
        os.mkdir(wp), os.mkdir(wt)
        old = side(os.path.join(tmp, PKG), ["art_kernels.hip"], wp)
        new = side(os.path.join(ROOT, PKG), ["art_trace.hip", "art_stages.hip", "art_frame.hip"], wt)
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", parent_rev], text=True).strip()
    rows, bad = [], 0
    for k in sorted(set(old) | set(new)):
        if k not in new or k not in old:
            rows.append("| `%s` | %s | | only in %s |" % (k, new[k][0] if k in new else "", "this tree" if k in new else "the parent"))
            bad += 1
            continue
        (_, told, rold), (unit, tnew, rnew) = old[k], new[k]
        same = told == tnew and rold == rnew and "?" not in rnew
        bad += not same
        regs = " / ".join(rnew) if rold == rnew else "parent " + " / ".join(rold) + ", this " + " / ".join(rnew)
        rows.append("| `%s` | `%s` | %s | %s |" % (k, unit, regs, "same" if same else "differs" + ("" if told == tnew else " (instructions)")))
    text = ["# The kernels are the parent's", "",
            "`compare.py`: `art_kernels.hip` of the parent (%s) against `art_trace.hip`, `art_stages.hip` and `art_frame.hip` of this tree, device side" % rev,
            "only, each with its Makefile's compile line.  registers = " + " / ".join(SHORT) + " of `-Rpass-analysis=kernel-resource-usage`;",
            "same = these figures, the instruction stream and the `.amdhsa_kernel` block are equal.  %d kernels in the parent, %d here, %d not the same." % (len(old), len(new), bad), "",
            "| kernel | unit | registers | |", "|---|---|---|---|"] + rows
    open(out_path, "w").write("\n".join(text) + "\n")
    print("%d kernels in the parent, %d here, %d not the same -> %s" % (len(old), len(new), bad, out_path))
    return 1 if bad else 0


def objects_table(parent_build, this_build, out_path):
    def sha(p):
        return hashlib.sha256(open(p, "rb").read()).hexdigest()
    names = sorted(n for n in os.listdir(this_build) if n.endswith(".hip.o") and os.path.exists(os.path.join(parent_build, n)))
    rows, bad = [], 0
    for n in names:
        a, b = sha(os.path.join(parent_build, n)), sha(os.path.join(this_build, n))
        bad += a != b
        rows.append("| `%s` | `%s` | `%s` | %s |" % (n, a, b, "same" if a == b else "differs"))
    text = ["# The other device objects are the parent's", "",
            "`compare.py --objects`: sha256 of the `build/*.hip.o` that exist at the parent and here, both built with the Makefile's flags.  %d of %d differ." % (bad, len(names)), "",
            "| object | parent | this commit | |", "|---|---|---|---|"] + rows
    open(out_path, "w").write("\n".join(text) + "\n")
    print("%d objects, %d differ -> %s" % (len(names), bad, out_path))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD~1")
    ap.add_argument("--objects", nargs=2, metavar=("PARENT_BUILD", "THIS_BUILD"))
    ap.add_argument("--out")
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    if a.objects:
        sys.exit(objects_table(a.objects[0], a.objects[1], a.out or os.path.join(here, "objects.md")))
    sys.exit(kernels_table(a.parent, a.out or os.path.join(here, "kernels.md")))
