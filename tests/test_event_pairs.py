"""The event-pair pool of the host driver (csrc/art_event_pairs.h) is host-only logic over six HIP calls: tests/event_pairs_check.cpp
exercises it against counting stubs of those calls.  Built as a stand-alone program with AddressSanitizer + UBSan and run on the CPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_event_pairs_host_logic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "event_pairs_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", os.path.join(HERE, "event_pairs_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("event pairs ok"), r.stdout + r.stderr
