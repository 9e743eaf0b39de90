"""art_aovs_rays_device and art_camera_rays_device without a GPU: declared in the header, exported by the library, listed in
EXPORTED_SYMBOLS and bound in Ada; the structs match the header as compiled; what can be refused without a device is, each with its
reason."""
import ctypes as C
import os
import re
import subprocess

NAMES = ("art_aovs_rays_device", "art_camera_rays_device")
BUFFERS = ("albedo3f", "normal3f", "position3f", "depth", "alpha", "prim_type", "prim_index", "mat")


def test_symbols_declared_exported_and_bound(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_aovs_rays_device\(const ArtAovRaysParams\* p, const float\* origins3f, const float\* dirs3f,\s*const float\* tnear\s*, "
                     r"const float\* tfar\s*, int64_t n_rays,\s*const ArtAovRayBuffers\* out, void\* hip_stream\);", hdr)
    assert re.search(r"int\s+art_camera_rays_device\(const ArtPassParams\* p, float\* origins3f, float\* dirs3f, void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, out, flags=re.M)
        assert name in art.EXPORTED_SYMBOLS and getattr(art.load_library(), name) is not None
        assert 'pragma Import (C, %s, "%s");' % (name, name) in ads
    assert hasattr(art.Backend, "aovs_rays_torch") and hasattr(art.Backend, "camera_rays_torch")


def test_structs_match_the_header_as_compiled(art, tmp_path):
    P, B = art.aov_rays.ArtAovRaysParams, art.aov_rays.ArtAovRayBuffers
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu", sizeof(ArtAovRaysParams), offsetof(ArtAovRaysParams, group), offsetof(ArtAovRaysParams, background), sizeof(ArtAovRayBuffers));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtAovRayBuffers, %s));\n' % n for n in BUFFERS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [16, 0, 4, 64] + [8 * i for i in range(8)]
    assert [C.sizeof(P), P.group.offset, P.background.offset, C.sizeof(B)] + [getattr(B, n).offset for n in BUFFERS] == got
    assert [n for n, _ in B._fields_] == list(BUFFERS)


def test_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call)"""
    L = art.load_library()
    one = C.c_void_p(16)                    # never dereferenced: every call below is refused on its parameters or the missing scene
    P, B = art.aov_rays.ArtAovRaysParams, art.aov_rays.ArtAovRayBuffers

    def buffers():
        b = B(); b.depth = 16
        return b

    def refused(text, p=P(4), n=8, o=one, d=one, out=buffers()):
        rc = L.art_aovs_rays_device(C.byref(p) if p is not None else None, o, d, None, None, n, C.byref(out) if out is not None else None, None)
        assert rc != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())
    refused("art_aovs_rays_device: null ArtAovRaysParams", p=None)
    refused("art_aovs_rays_device: null ArtAovRayBuffers", out=None)
    refused("all eight pointers are null", out=B())
    refused("group must be 1..16", p=P(0))
    refused("group must be 1..16", p=P(17))
    refused("group must be 1..16", p=P(-4))
    refused("n_rays must be 0 .. 2^31 - 1", n=-4)
    refused("n_rays must be 0 .. 2^31 - 1", n=1 << 31)
    refused("is not a multiple of group 4", n=6)
    refused("is not a multiple of group 16", p=P(16), n=(1 << 31) - 1)
    refused("null origins3f or dirs3f", o=None)
    refused("null origins3f or dirs3f", d=None)
    # past the parameters: no scene -- or, where an earlier test of the same process left one on a GPU, the pointer check
    assert L.art_aovs_rays_device(C.byref(P(4)), one, one, None, None, 8, C.byref(buffers()), None) != 0
    assert any(t in L.art_last_error().decode() for t in ("no scene uploaded", "is not device memory"))
    # n_rays == 0 succeeds and touches nothing, whatever the pointers ... but not with parameters that are refused
    assert L.art_aovs_rays_device(C.byref(P(4)), None, None, None, None, 0, C.byref(buffers()), None) == 0
    refused("group must be 1..16", p=P(0), n=0)
    pp = art.Backend.pass_params()
    assert L.art_camera_rays_device(None, one, one, None) != 0 and "art_camera_rays_device: null ArtPassParams" in L.art_last_error().decode()
    assert L.art_camera_rays_device(C.byref(pp), None, one, None) != 0 and "null origins3f or dirs3f" in L.art_last_error().decode()
    assert L.art_camera_rays_device(C.byref(pp), one, None, None) != 0 and "null origins3f or dirs3f" in L.art_last_error().decode()
    assert L.art_camera_rays_device(C.byref(pp), one, one, None) != 0
    assert any(t in L.art_last_error().decode() for t in ("no scene uploaded", "no viewport", "is not device memory"))
