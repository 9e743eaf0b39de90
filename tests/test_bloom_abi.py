"""art_bloom_device without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in Ada; the
struct matches the header as compiled; what can be refused without a device is, each with its message
(tests/golden/bloom_refusals.json); and the Python entry checks its tensors before any C call."""
import ctypes as C
import os
import re
import subprocess

import pytest

import bloom_refusals as RF

NAME = "art_bloom_device"
FIELDS = ("width", "height", "levels", "karis", "variant", "scale", "exposure", "threshold", "knee", "scatter", "strength")


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_bloom_device\(const ArtBloomParams\* p, const float\* color3f, const void\* exposure_state\s*,\s*"
                     r"float\* out3f\s*, float\* bloom3f\s*, void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert NAME in art.EXPORTED_SYMBOLS and getattr(art.load_library(), NAME) is not None
    assert re.search(r"\bT %s$" % NAME, out, flags=re.M)
    assert 'pragma Import (C, %s, "%s");' % (NAME, NAME) in open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert hasattr(art.Backend, "bloom_torch")


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtBloomParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtBloomParams, %s));\n' % n for n in FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [44] + [4 * k for k in range(11)]
    bp = art.bloom.ArtBloomParams
    assert got == want and [C.sizeof(bp)] + [getattr(bp, n).offset for n in FIELDS] == want
    assert [n for n, _ in bp._fields_] == list(FIELDS) and [t for _, t in bp._fields_] == [C.c_int32] * 5 + [C.c_float] * 6


def test_the_defaults_are_the_conventional_ones(art):
    b = art.bloom
    assert (b.BLOOM_LEVELS, b.BLOOM_SCATTER, b.BLOOM_STRENGTH, b.BLOOM_THRESHOLD, b.BLOOM_KNEE, b.BLOOM_KARIS) == (6, 0.7, 0.05, 0.0, 0.0, 1)
    assert b.BLOOM_VARIANT in (0, 1) and "not the result of a sweep" in open(os.path.join(art.PKG_DIR, "bloom.py")).read().lower()


def test_refusals_that_need_no_device(art):
    """the parameter and overlap checks come before the device is looked for: each names its reason (no GPU is touched by a refused
    call; the pointers are never dereferenced)"""
    L = art.load_library()
    frame, cases = RF.load()
    base = {k: (1 << 30) + (i << 24) for i, k in enumerate(RF.PLANES)}
    early = [c for c in cases if not c["needs_device"]]
    assert len(early) >= 30 and len(early) < len(cases)
    for case in early:
        RF.check(art, L, frame, case, base, host=1 << 20, short=lambda n: 1 << 22)
    # what passes every one of these stops at the next check (no device here, or the pointers are no device memory), not at a parameter
    for extra in (dict(levels=8, karis=0, variant=1, threshold=0.0, knee=0.0, scatter=0.0, strength=1.0), dict(levels=1, scatter=1.0, strength=0.0, exposure=0.0)):
        rc, text = RF.call(art, L, frame, dict(name="good", set=extra), base)
        assert rc != 0 and not any(t in text for t in ("must be", "null", "overlaps", "not finite")), text
    rc, text = RF.call(art, L, frame, dict(name="in place", args={"out3f": "is color3f"}), base)
    assert rc != 0 and not any(t in text for t in ("must be", "null", "overlaps", "not finite")), text


def test_the_fixture_covers_every_plane(art):
    """per plane: on the host, one pixel short, an overlap, and a bad parameter next to a bad plane"""
    _, cases = RF.load()
    for plane in RF.PLANES:
        hows = [(c["args"].get(plane, ""), "set" in c) for c in cases if plane in c.get("args", {})]
        assert ("host", False) in hows and ("short", False) in hows, plane
        assert any(s and h in ("host", "short") for h, s in hows), plane
        assert any(h.startswith(("over ", "is ")) for h, _ in hows) or any(a in ("over " + plane, "is " + plane) for c in cases for a in c.get("args", {}).values()), plane


def test_python_refuses_bad_tensors_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    f = be.bloom_torch
    color, state = torch.zeros(6, 8, 3), torch.zeros(260, dtype=torch.int32)
    with pytest.raises(art.ArtError, match="color: a torch tensor"):
        f(None)
    with pytest.raises(art.ArtError, match=r"color: shape must be \[H, W, 3\]"):
        f(torch.zeros(6, 8))
    with pytest.raises(art.ArtError, match="color: dtype"):
        f(color.double())
    with pytest.raises(art.ArtError, match="exposure_state: dtype"):
        f(color, torch.zeros(260))
    with pytest.raises(art.ArtError, match="exposure_state: shape"):
        f(color, torch.zeros(259, dtype=torch.int32))
    with pytest.raises(art.ArtError, match="out: shape"):
        f(color, state, out=torch.zeros(6, 9, 3))
    with pytest.raises(art.ArtError, match="bloom_out: dtype"):
        f(color, state, bloom_out=color.double())
    with pytest.raises(art.ArtError, match="bloom_out: shape"):
        f(color, state, bloom_out=torch.zeros(8, 6, 3))
    with pytest.raises(art.ArtError, match="contiguous"):
        f(torch.zeros(8, 6, 3).transpose(0, 1), state)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(color, state)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(color)
