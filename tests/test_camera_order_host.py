"""The order in which bounce 0 visits a batch's path slots with option camera_order = 1 (csrc/art_camera_order.h), without a GPU:
tests/camera_order_host is a stand-alone g++ program over the header, built with AddressSanitizer and UBSan and run as a process of its
own.  It prints the units of the order; what the order must be is checked here, from the definition and not from the header's arithmetic:
  unit   256 consecutive slots of one sample row (slot = s * pn + pl): pixels [256 q, min(256 q + 256, pn)) of sample s;
  block  1024 consecutive pl (four units of a row; the last block of a row and its last unit may be partial);
  order  block-major, then sample, then the block's units;
  the visiting space is 256 positions per unit and sn * ceil(pn / 256) units, its positions past a unit's slots are padding."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PROG = os.path.join(HERE, "camera_order_host", "camera_order_host")

SHAPES = [(1, 4), (255, 4), (256, 8), (257, 4), (1024, 4), (1025, 8), (1920, 8), (2560, 1), (3000, 12)]      # (pn, sn)


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(PROG)])
    return PROG


def units_of(prog, pn, sn):
    r = subprocess.run([prog, str(pn), str(sn)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]          # (a sanitizer report ends the program with a status of its own)
    lines = r.stdout.split("\n")
    n = int(lines[0].split()[1])
    units = [tuple(int(x) for x in l.split()[1:]) for l in lines[1:1 + n]]
    tail = lines[1 + n].split()
    assert lines[0].startswith("units ") and tail[0] == "positions" and tail[2] == "unmasked" and all(l.startswith("u ") for l in lines[1:1 + n])
    return units, int(tail[1]), int(tail[3])


def test_the_programs_own_checks(prog):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "camera_order_host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("pn, sn", SHAPES)
def test_the_order(prog, pn, sn):
    units, positions, unmasked = units_of(prog, pn, sn)
    # the visiting space: one unit per 256 pixels (or what is left of them) of every sample row, 256 positions each -- nothing more
    row_units = (pn + 255) // 256
    assert len(units) == sn * row_units and positions == 256 * sn * row_units and unmasked == pn * sn
    # the unmasked positions map one-to-one onto [0, pn * sn)
    slots = [s for slot0, count in units for s in range(slot0, slot0 + count)]
    assert len(slots) == pn * sn and sorted(slots) == list(range(pn * sn))
    # every unit is THE unit of the definition: consecutive slots of one sample row, from a multiple of 256 pixels to the next or to pn
    keys = []
    for slot0, count in units:
        s, pl0 = divmod(slot0, pn)
        assert 0 <= s < sn and pl0 % 256 == 0 and count == min(256, pn - pl0) and 1 <= count
        assert (slot0 + count - 1) // pn == s
        keys.append((pl0 // 1024, s, pl0))
    # all positions of a block come before any position of the next block; inside a block sample by sample; inside a sample its units in order
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    blocks = [k[0] for k in keys]
    assert blocks == sorted(blocks) and set(blocks) == set(range((pn + 1023) // 1024))
    for b in set(blocks):                                  # a block: every sample's units of its pixels, together
        want = sn * ((min(pn, 1024 * b + 1024) - 1024 * b + 255) // 256)
        assert blocks.count(b) == want and blocks.index(b) + want - 1 == len(blocks) - 1 - blocks[::-1].index(b)


def test_the_option_is_registered():
    """art_set_option("camera_order"): 0 and 1 are taken, anything else is refused with the option's text (no device is touched; a child
    process, because the library's options are process-wide)"""
    child = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; L = g.load_package().load_library()\n"
             "for v in (-1, 0, 1, 2): print(v, L.art_set_option(b'camera_order', v), L.art_last_error().decode() if v in (-1, 2) else '')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split(" ", 2) for l in r.stdout.strip().split("\n")]
    assert [(int(a), int(b) == 0) for a, b, _ in rows] == [(-1, False), (0, True), (1, True), (2, False)]
    assert all(t.startswith("camera_order: 0 ") for a, b, t in rows if int(b) != 0)
