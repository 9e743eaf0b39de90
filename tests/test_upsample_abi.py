"""art_upsample_device without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in Ada; the
structs match the header as compiled; what can be refused without a device is, each with its message; and the Python entry checks its
tensors before any C call."""
import ctypes as C
import os
import re
import subprocess

import pytest

NAME = "art_upsample_device"
PARAM_FIELDS = ("width", "height", "lo_width", "lo_height", "footprint", "demodulate", "normal_log2", "scale", "sigma_depth", "jitter")
GUIDE_FIELDS = ("albedo3f", "normal3f", "depth", "id")
GOOD = dict(width=8, height=6, lo_width=4, lo_height=3, footprint=2, demodulate=0, normal_log2=5, scale=1.0, sigma_depth=1.0, jitter=(0.0, 0.0))


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_upsample_device\(const ArtUpsampleParams\* p, const float\* lo_color3f, const ArtUpsampleGuides\* lo, const ArtUpsampleGuides\* hi,\s*"
                     r"float\* out3f, uint8_t\* fallback1b\s*, void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert NAME in art.EXPORTED_SYMBOLS and getattr(art.load_library(), NAME) is not None
    assert re.search(r"\bT %s$" % NAME, out, flags=re.M)
    assert 'pragma Import (C, %s, "%s");' % (NAME, NAME) in open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert hasattr(art.Backend, "upsample_torch")


def test_structs_match_the_header_as_compiled(art, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtUpsampleParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtUpsampleParams, %s));\n' % n for n in PARAM_FIELDS)
                   + '  printf(" %zu", sizeof(ArtUpsampleGuides));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtUpsampleGuides, %s));\n' % n for n in GUIDE_FIELDS)
                   + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want_p, want_g = [44] + [4 * k for k in range(10)], [32, 0, 8, 16, 24]
    assert got == want_p + want_g
    up, ug = art.upsample.ArtUpsampleParams, art.upsample.ArtUpsampleGuides
    assert [C.sizeof(up)] + [getattr(up, n).offset for n in PARAM_FIELDS] == want_p
    assert [C.sizeof(ug)] + [getattr(ug, n).offset for n in GUIDE_FIELDS] == want_g
    assert [t for _, t in up._fields_] == [C.c_int32] * 7 + [C.c_float] * 2 + [C.c_float * 2]
    assert [t for _, t in ug._fields_] == [C.c_void_p] * 4


def test_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call)"""
    L = art.load_library()
    color, out, plane = 1 << 20, 1 << 30, 1 << 24                      # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")
    U = art.upsample

    def guides(**kw):
        return U.ArtUpsampleGuides(*[kw.get(n) for n in GUIDE_FIELDS])

    def refused(text, color=color, out=out, lo=guides(), hi=guides(), null_params=False, **kw):
        v = dict(GOOD, **kw)
        par = U.ArtUpsampleParams(*[v[n] if n != "jitter" else (C.c_float * 2)(*v[n]) for n in PARAM_FIELDS])
        rc = L.art_upsample_device(None if null_params else C.byref(par), color, None if lo is None else C.byref(lo), None if hi is None else C.byref(hi), out, None, None)
        msg = L.art_last_error().decode()
        assert rc != 0 and msg.startswith("art_upsample_device: ") and text in msg, (text, msg)
    refused("null ArtUpsampleParams", null_params=True)
    refused("null lo_color3f or out3f", color=None)
    refused("null lo_color3f or out3f", out=None)
    refused("null ArtUpsampleGuides", lo=None)
    refused("null ArtUpsampleGuides", hi=None)
    refused("width and height must be at least 1", width=0, lo_width=0)
    refused("width and height must be at least 1", height=-3)
    refused("at most 2^28", width=1 << 15, height=1 << 14)
    refused("lo_width must be 1 .. width", lo_width=0)
    refused("lo_width must be 1 .. width", lo_width=9)
    refused("lo_height 1 .. height", lo_height=0)
    refused("lo_height 1 .. height", lo_height=7)
    for fp in (0, 1, 3, 5, -2):
        refused("footprint must be 2 or 4", footprint=fp)
    refused("normal_log2 must be 0 .. 10", normal_log2=-1)
    refused("normal_log2 must be 0 .. 10", normal_log2=11)
    refused("scale is not finite", scale=inf)
    refused("scale is not finite", scale=nan)
    refused("sigma_depth is NaN", sigma_depth=nan)
    for j in ((0.5, 0.0), (0.0, -0.5), (nan, 0.0), (0.0, inf), (-0.75, 0.0)):
        refused("each jitter must be inside (-0.5, 0.5)", jitter=j)
    for k, n in enumerate(GUIDE_FIELDS):
        what = "%s is given on one side only" % n
        refused(what, lo=guides(**{n: plane}))
        refused(what, hi=guides(**{n: plane}))
    refused("demodulate needs the albedo planes", demodulate=1)
    refused("demodulate needs the albedo planes", demodulate=1, lo=guides(normal3f=plane), hi=guides(normal3f=plane))
    # what passes every one of these stops at the next check (no device here, or the pointers are no device memory), not at a parameter
    par = U.ArtUpsampleParams(*[GOOD[n] if n != "jitter" else (C.c_float * 2)(0.49, -0.49) for n in PARAM_FIELDS])
    g = guides(albedo3f=plane)
    assert L.art_upsample_device(C.byref(par), color, C.byref(g), C.byref(g), out, None, None) != 0
    assert not any(t in L.art_last_error().decode() for t in ("jitter", "one side", "must be", "null "))


def test_python_refuses_bad_tensors_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    f = be.upsample_torch
    lo_color = torch.zeros(3, 4, 3)
    lo = dict(albedo=torch.zeros(3, 4, 3), normal=torch.zeros(3, 4, 3), depth=torch.zeros(3, 4), id=torch.zeros(3, 4, dtype=torch.int32))
    hi = dict(albedo=torch.zeros(6, 8, 3), normal=torch.zeros(6, 8, 3), depth=torch.zeros(6, 8), id=torch.zeros(6, 8, dtype=torch.int32))
    with pytest.raises(art.ArtError, match="color: a torch tensor"):
        f(None, lo, hi)
    with pytest.raises(art.ArtError, match=r"color: shape must be \[H, W, 3\]"):
        f(torch.zeros(3, 4), lo, hi)
    with pytest.raises(art.ArtError, match="lo_color: dtype"):
        f(lo_color.double(), lo, hi)
    with pytest.raises(art.ArtError, match="lo_guides: a dict of planes is required"):
        f(lo_color, None, hi)
    with pytest.raises(art.ArtError, match="hi_guides: a dict of planes is required"):
        f(lo_color, lo, [1])
    with pytest.raises(art.ArtError, match="depth is given on one side only"):
        f(lo_color, dict(lo, depth=None), hi)
    with pytest.raises(art.ArtError, match="id is given on one side only"):
        f(lo_color, lo, {k: v for k, v in hi.items() if k != "id"})
    with pytest.raises(art.ArtError, match=r"lo_guides\['normal'\]: shape"):
        f(lo_color, dict(lo, normal=torch.zeros(3, 5, 3)), hi)
    with pytest.raises(art.ArtError, match=r"hi_guides\['depth'\]: shape"):
        f(lo_color, lo, dict(hi, depth=torch.zeros(6, 8, 1)))
    with pytest.raises(art.ArtError, match=r"hi_guides\['id'\]: dtype"):
        f(lo_color, lo, dict(hi, id=torch.zeros(6, 8)))
    with pytest.raises(art.ArtError, match=r"lo_guides\['albedo'\]: dtype"):
        f(lo_color, dict(lo, albedo=lo["albedo"].half()), hi)
    with pytest.raises(art.ArtError, match="contiguous"):
        f(lo_color, lo, dict(hi, depth=torch.zeros(8, 6).t()))
    with pytest.raises(art.ArtError, match="contiguous"):
        f(torch.zeros(4, 3, 3).transpose(0, 1), lo, hi)
    with pytest.raises(art.ArtError, match="out: shape"):
        f(lo_color, lo, hi, out=torch.zeros(6, 9, 3))
    with pytest.raises(art.ArtError, match="out: dtype"):
        f(lo_color, {}, {}, out=torch.zeros(6, 8, 3, dtype=torch.float64))
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(lo_color, lo, hi)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(lo_color, {}, {})
