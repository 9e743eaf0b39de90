"""art_svgf_spatial_variance_device without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound
in Ada; the struct matches the header as compiled; what can be refused without a device is, each with its message; and the Python
entry checks its tensors before any C call."""
import ctypes as C
import os
import re
import subprocess

import pytest

NAME = "art_svgf_spatial_variance_device"
FIELDS = ("width", "height", "radius", "normal_log2", "min_history", "sigma_depth")


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_svgf_spatial_variance_device\(const ArtSvgfSpatialParams\* p, const void\* hist, const float\* variance_in1f, float\* variance_out1f,\s*"
                     r"void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert NAME in art.EXPORTED_SYMBOLS and getattr(art.load_library(), NAME) is not None
    assert re.search(r"\bT %s$" % NAME, out, flags=re.M)
    assert 'pragma Import (C, %s, "%s");' % (NAME, NAME) in ads


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtSvgfSpatialParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtSvgfSpatialParams, %s));\n' % n for n in FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [24, 0, 4, 8, 12, 16, 20]
    assert got == want
    par = art.ArtSvgfSpatialParams
    assert [C.sizeof(par)] + [getattr(par, n).offset for n in FIELDS] == want
    assert [t for _, t in par._fields_] == [C.c_int32] * 4 + [C.c_float] * 2


def test_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call)"""
    L = art.load_library()
    hist, vin, vout = C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(1 << 31)       # never dereferenced: every call below is refused

    def refused(text, p=(4, 4, 3, 7, 4.0, 1.0), hist=hist, vin=vin, vout=vout):
        par = art.ArtSvgfSpatialParams(*p) if p is not None else None
        rc = L.art_svgf_spatial_variance_device(C.byref(par) if par is not None else None, hist, vin, vout, None)
        msg = L.art_last_error().decode()
        assert rc != 0 and msg.startswith(NAME + ": ") and text in msg, (text, msg)
    refused("null ArtSvgfSpatialParams", p=None)
    refused("null hist, variance_in1f or variance_out1f", hist=None)
    refused("null hist, variance_in1f or variance_out1f", vin=None)
    refused("null hist, variance_in1f or variance_out1f", vout=None)
    refused("width and height must be at least 1", p=(0, 4, 3, 7, 4.0, 1.0))
    refused("width and height must be at least 1", p=(4, -1, 3, 7, 4.0, 1.0))
    refused("at most 2^28", p=(1 << 15, 1 << 14, 3, 7, 4.0, 1.0))
    refused("radius must be 1 .. 3", p=(4, 4, 0, 7, 4.0, 1.0))
    refused("radius must be 1 .. 3", p=(4, 4, 4, 7, 4.0, 1.0))
    refused("normal_log2 must be 0 .. 10", p=(4, 4, 3, -1, 4.0, 1.0))
    refused("normal_log2 must be 0 .. 10", p=(4, 4, 3, 11, 4.0, 1.0))
    refused("min_history or sigma_depth is NaN", p=(4, 4, 3, 7, float("nan"), 1.0))
    refused("min_history or sigma_depth is NaN", p=(4, 4, 3, 7, 4.0, float("nan")))
    n = 16
    refused("variance_out1f overlaps hist", vout=C.c_void_p(hist.value))
    refused("variance_out1f overlaps hist", vout=C.c_void_p(hist.value + 48 * n - 4))
    refused("variance_out1f overlaps hist", vout=C.c_void_p(hist.value - 4 * n + 4))


def test_python_refuses_bad_tensors_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    hist, var = torch.zeros(3, 4, 5, 4), torch.zeros(4, 5)
    f = be.svgf_spatial_variance_torch
    with pytest.raises(art.ArtError, match="hist: a torch tensor"):
        f(None, var, 5, 4)
    with pytest.raises(art.ArtError, match="variance: a torch tensor"):
        f(hist, None, 5, 4)
    with pytest.raises(art.ArtError, match="hist: shape"):
        f(hist, var, 4, 5)
    with pytest.raises(art.ArtError, match="variance: shape"):
        f(hist, torch.zeros(4, 5, 1), 5, 4)
    with pytest.raises(art.ArtError, match="out: shape"):
        f(hist, var, 5, 4, out=torch.zeros(5, 4))
    with pytest.raises(art.ArtError, match="variance: dtype"):
        f(hist, var.double(), 5, 4)
    with pytest.raises(art.ArtError, match="contiguous"):
        f(hist, torch.zeros(5, 4).t(), 5, 4)
    with pytest.raises(art.ArtError, match="width and height"):
        f(hist, var, 0, 4)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(hist, var, 5, 4)
