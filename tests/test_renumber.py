"""The renumbering of a GPU-built tree into the host builder's numbering (csrc/art_renumber.h) is host-only logic:
tests/renumber_check.cpp shuffles the host builder's trees of a 2-, 5-, 300- and 2000-triangle mesh and demands them back byte for
byte, and demands that broken trees are refused.  Built as a stand-alone program, plain and with AddressSanitizer + UBSan, and run on the CPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ada-ray-tracer_amd", "csrc")
COMMON = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", os.path.join(HERE, "..", "include"),
          os.path.join(HERE, "renumber_check.cpp"), os.path.join(CSRC, "art_bvh.cpp"), "-lpthread"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                             "-static-libasan", "-static-libubsan"]], ids=["plain", "sanitizers"])
def test_renumbering_gives_the_host_builders_tree(tmp_path, flags):
    exe = str(tmp_path / "renumber_check")
    subprocess.check_call(COMMON + flags + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("renumber ok"), r.stdout + r.stderr
