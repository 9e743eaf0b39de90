"""art_radiance_rays_device without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in Ada;
ArtRadianceParams matches the header as compiled; what can be refused without a device is, each with its reason; the Python layer
refuses bad tensors before any C call."""
import ctypes as C
import os
import re
import subprocess

import pytest

NAME = "art_radiance_rays_device"
FIELDS = ("render_type", "max_depth", "samples", "sample_base", "seed")


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_radiance_rays_device\(const ArtRadianceParams\* p, const float\* origins3f, const float\* dirs3f, const uint32_t\* keys1u\s*, int64_t n,\s*"
                     r"float\* radiance3f, float\* moments2f\s*\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert re.search(r"\bT %s$" % NAME, out, flags=re.M)
    assert [l.split()[-1] for l in out.splitlines() if "radiance" in l and " T art_" in l] == [NAME]      # the one new C symbol
    assert NAME in art.EXPORTED_SYMBOLS and getattr(art.load_library(), NAME) is not None
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert 'pragma Import (C, %s, "%s");' % (NAME, NAME) in ads
    assert hasattr(art.Backend, "radiance_rays_torch")


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtRadianceParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtRadianceParams, %s));\n' % n for n in FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [24, 0, 4, 8, 12, 16]
    assert got == want
    assert [C.sizeof(art.radiance.ArtRadianceParams)] + [getattr(art.radiance.ArtRadianceParams, n).offset for n in FIELDS] == want


def test_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call)"""
    L = art.load_library()
    one = C.c_void_p(16)                    # never dereferenced: every call below is refused on its parameters or the missing scene

    def refused(p, text, n=4, o=one, d=one, out=one):
        rc = L.art_radiance_rays_device(C.byref(p) if p is not None else None, o, d, None, n, out, None)
        assert rc != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())

    def params(**kw):
        p = art.radiance.ArtRadianceParams(art.PT_MIS, 8, 1, 0, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    refused(None, NAME + ": null ArtRadianceParams")
    refused(params(render_type=art.RT_DEBUG), "debug render types")
    refused(params(render_type=art.RT_WHITTED), "debug render types")
    refused(params(render_type=5), "unknown render_type")
    refused(params(render_type=-1), "unknown render_type")
    refused(params(max_depth=0), "max_depth must be 1..16")
    refused(params(max_depth=17), "max_depth must be 1..16")
    refused(params(samples=0), "samples must be >= 1")
    refused(params(samples=-3), "samples must be >= 1")
    refused(params(), "n must be 0 .. 2^28", n=-1)
    refused(params(), "n must be 0 .. 2^28", n=(1 << 28) + 1)
    refused(params(), "null origins3f, dirs3f or radiance3f", o=None)
    refused(params(), "null origins3f, dirs3f or radiance3f", d=None)
    refused(params(), "null origins3f, dirs3f or radiance3f", out=None)
    # past the parameters: no scene -- or, where an earlier test of the same process left one on a GPU, the pointer check
    assert L.art_radiance_rays_device(C.byref(params()), one, one, None, 4, one, None) != 0
    assert any(t in L.art_last_error().decode() for t in ("no scene uploaded", "is not device memory"))
    # n == 0 succeeds and touches nothing, whatever the pointers
    assert L.art_radiance_rays_device(C.byref(params()), None, None, None, 0, None, None) == 0
    # ... but not with parameters that are refused
    refused(params(samples=0), "samples must be >= 1", n=0)


def test_python_refuses_bad_tensors_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    o = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(art.ArtError, match="origins: a \\[N, 3\\] float32 tensor"):
        be.radiance_rays_torch([[0, 0, 0]], o)
    with pytest.raises(art.ArtError, match="origins: dtype"):
        be.radiance_rays_torch(o.double(), o)
    with pytest.raises(art.ArtError, match="origins: shape"):
        be.radiance_rays_torch(torch.zeros((4, 4)), torch.zeros((4, 4)))
    with pytest.raises(art.ArtError, match="dirs: shape"):
        be.radiance_rays_torch(o, torch.zeros((5, 3)))
    with pytest.raises(art.ArtError, match="keys: dtype"):
        be.radiance_rays_torch(o, o, keys=torch.zeros(4))
    with pytest.raises(art.ArtError, match="keys: shape"):
        be.radiance_rays_torch(o, o, keys=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(art.ArtError, match="out: shape"):
        be.radiance_rays_torch(o, o, out=torch.zeros((3, 3)))
    with pytest.raises(art.ArtError, match="out: the tensor must be contiguous"):
        be.radiance_rays_torch(o, o, out=torch.zeros((4, 6))[:, ::2])
    with pytest.raises(art.ArtError, match="moments: shape"):
        be.radiance_rays_torch(o, o, moments=torch.zeros((4, 3)))
    with pytest.raises(art.ArtError, match="origins: must be a GPU tensor"):
        be.radiance_rays_torch(o, o)
