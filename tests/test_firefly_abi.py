"""art_firefly_device without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in Ada; the
struct matches the header as compiled; what can be refused without a device is, each with its message
(tests/golden/firefly_refusals.json); and the Python entry checks its tensors before any C call."""
import ctypes as C
import os
import re
import subprocess

import pytest

import firefly_refusals as RF

NAME = "art_firefly_device"
FIELDS = ("width", "height", "radius", "rank", "min_count", "scale", "gain", "floor")


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_firefly_device\(const ArtFireflyParams\* p, const float\* color3f, const float\* moments2f\s*, const int32_t\* id\s*,\s*"
                     r"float\* out3f, float\* moments_out2f\s*, uint8_t\* clamped1b\s*,\s*void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert NAME in art.EXPORTED_SYMBOLS and getattr(art.load_library(), NAME) is not None
    assert re.search(r"\bT %s$" % NAME, out, flags=re.M)
    assert 'pragma Import (C, %s, "%s");' % (NAME, NAME) in open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert hasattr(art.Backend, "firefly_torch")


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtFireflyParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtFireflyParams, %s));\n' % n for n in FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [32] + [4 * k for k in range(8)]
    fp = art.firefly.ArtFireflyParams
    assert got == want and [C.sizeof(fp)] + [getattr(fp, n).offset for n in FIELDS] == want
    assert [n for n, _ in fp._fields_] == list(FIELDS) and [t for _, t in fp._fields_] == [C.c_int32] * 5 + [C.c_float] * 3


def test_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call; the
    pointers are never dereferenced)"""
    L = art.load_library()
    frame, cases = RF.load()
    base = {k: (1 << 30) + (i << 24) for i, k in enumerate(RF.PLANES)}
    early = [c for c in cases if not c["needs_device"]]
    assert len(early) >= 20 and len(early) < len(cases)
    for case in early:
        RF.check(art, L, frame, case, base, host=1 << 20, short=lambda n: 1 << 22)
    # what passes every one of these stops at the next check (no device here, or the pointers are no device memory), not at a parameter
    rc, text = RF.call(art, L, frame, dict(name="good", set=dict(radius=1, rank=4, min_count=8, gain=1.0, floor=0.0)), base)
    assert rc != 0 and not any(t in text for t in ("must be", "null ", "without", "not finite"))


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
    f = be.firefly_torch
    color, moments, ids = torch.zeros(6, 8, 3), torch.zeros(6, 8, 2), torch.zeros(6, 8, dtype=torch.int32)
    with pytest.raises(art.ArtError, match="color: a torch tensor"):
        f(None)
    with pytest.raises(art.ArtError, match=r"color: shape must be \[H, W, 3\]"):
        f(torch.zeros(6, 8))
    with pytest.raises(art.ArtError, match="color: dtype"):
        f(color.double())
    with pytest.raises(art.ArtError, match="moments_out is given without moments"):
        f(color, moments_out=moments)
    with pytest.raises(art.ArtError, match="moments: shape must hold at least 96 elements"):
        f(color, torch.zeros(6, 7, 2))
    with pytest.raises(art.ArtError, match="moments: dtype"):
        f(color, moments.half())
    with pytest.raises(art.ArtError, match="id: dtype"):
        f(color, moments, torch.zeros(6, 8))
    with pytest.raises(art.ArtError, match="id: shape"):
        f(color, moments, torch.zeros(6, 8, 1, dtype=torch.int32))
    with pytest.raises(art.ArtError, match="out: shape"):
        f(color, moments, ids, out=torch.zeros(6, 9, 3))
    with pytest.raises(art.ArtError, match="moments_out: dtype"):
        f(color, moments, ids, moments_out=moments.double())
    with pytest.raises(art.ArtError, match="contiguous"):
        f(torch.zeros(8, 6, 3).transpose(0, 1), moments, ids)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(color, moments, ids)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(color)
