"""First-hit feature buffers without a GPU: art_render_aovs_device is declared and exported, ArtAovBuffers matches the header as
compiled, the call is refused with a message before anything could be launched, and render_aovs_torch validates `want` on the host."""
import ctypes as C
import os
import re
import subprocess

import pytest

FIELDS = ("albedo3f", "normal3f", "depth", "alpha", "prim_type", "prim_index", "mat")


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    assert re.search(r"int\s+art_render_aovs_device\(const ArtPassParams\* p, const ArtAovBuffers\* out, void\* hip_stream\);", hdr)
    assert "art_render_aovs_device" in art.EXPORTED_SYMBOLS
    assert getattr(L, "art_render_aovs_device") is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert re.search(r"\bT art_render_aovs_device$", out, flags=re.M)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert 'pragma Import (C, art_render_aovs_device, "art_render_aovs_device");' in ads


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    """sizeof / offsetof from a C compiler reading include/art_hip.h against the ctypes mirror: 56 bytes, seven pointers in the header's order"""
    B = art.ArtAovBuffers
    assert [name for name, _ in B._fields_] == list(FIELDS)
    assert C.sizeof(B) == 56 and [getattr(B, name).offset for name in FIELDS] == [0, 8, 16, 24, 32, 40, 48]
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtAovBuffers));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtAovBuffers, %s));\n' % name for name in FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(B)] + [getattr(B, name).offset for name in FIELDS]
    assert C.sizeof(art.ArtPassParams) == 48 and C.sizeof(art.ArtHit) == 44      # the structs next to it are left as they were


def test_refused_with_a_message_before_anything_is_launched(art):
    """In a process of its own, where no scene was ever uploaded: every refusal below comes from the argument checks, in the header's order
    (arguments, then the scene), whether or not the machine has a device."""
    import sys
    code = ("import sys, ctypes as C; sys.path.insert(0, %r); import __graft_entry__ as g; art = g.load_package(); L = art.load_library()\n"
            "p = art.Backend.pass_params(); buf = art.ArtAovBuffers(); buf.depth = 0x1000      # never dereferenced: the call is refused first\n"
            "for args in ((C.byref(p), C.byref(buf)), (C.byref(p), None), (None, C.byref(buf)), (C.byref(p), C.byref(art.ArtAovBuffers()))):\n"
            "    print(L.art_render_aovs_device(args[0], args[1], None), L.art_last_error().decode())\n") % art.ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300).stdout.splitlines()
    assert len(out) == 4 and all(line.split()[0] != "0" for line in out), out
    assert "art_render_aovs_device: no scene uploaded" in out[0]
    assert "art_render_aovs_device: null ArtAovBuffers" in out[1]
    assert "art_render_aovs_device: null ArtPassParams" in out[2]
    assert "all seven pointers are null" in out[3]


def test_an_unknown_plane_raises_before_any_call(art):
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    with pytest.raises(ValueError, match="nope"):
        be.render_aovs_torch(art.Backend.pass_params(), want=("nope",))
    with pytest.raises(ValueError, match="unknown plane"):
        be.render_aovs_torch(art.Backend.pass_params(), want=("depth", "Alpha"))
    assert tuple(art.AOV_PLANES) == ("albedo", "normal", "depth", "alpha", "prim_type", "prim_index", "mat")
