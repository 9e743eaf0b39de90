"""The motion plane's ABI without a GPU: art_render_aovs_motion_device and art_temporal_motion_device are declared and exported,
ArtMotionSource matches the header as compiled, the structs next to it are what they were, and the calls are refused with a message
before anything could be launched."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

FIELDS = ("cur_pos3f", "prev_pos3f", "nverts", "prev_m12f", "n_instances")
SYMBOLS = ("art_render_aovs_motion_device", "art_temporal_motion_device")


def test_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert ("int art_render_aovs_motion_device(const ArtPassParams* p, const ArtAovBuffers* out, const ArtMotionSource* src, float* motion3f, "
            "void* hip_stream);") in hdr
    assert ("int art_temporal_motion_device(const ArtTemporalParams* p, const float* color3f, const float* moments2f, const float* normal3f, "
            "const float* depth, const int32_t* id, const float* motion3f, const void* hist_in, void* hist_out, float* out3f, "
            "float* variance_out, float* length_out, void* hip_stream);") in hdr
    L = art.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    for name in SYMBOLS:
        assert name in art.EXPORTED_SYMBOLS and getattr(L, name) is not None
        assert re.search(r"\bT %s$" % name, out, flags=re.M)
        assert 'pragma Import (C, %s, "%s");' % (name, name) in ads


def test_structs_match_the_header_as_compiled(art, tmp_path):
    """sizeof / offsetof from a C compiler reading include/art_hip.h against the ctypes mirror; ArtAovBuffers is still 56 bytes and
    ArtTemporalParams is what it was (2 x 84 + 20)"""
    S = art.ArtMotionSource
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert C.sizeof(S) == 40 and [getattr(S, name).offset for name in FIELDS] == [0, 8, 16, 24, 32]
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtMotionSource));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtMotionSource, %s));\n' % name for name in FIELDS)
                   + '  printf(" %zu %zu %zu %zu", sizeof(ArtAovBuffers), sizeof(ArtTemporalParams), sizeof(ArtTemporalCamera), offsetof(ArtTemporalParams, n_colours));\n'
                   + '  printf(" %zu", offsetof(ArtTemporalParams, normal_min));\n  return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:6] == [C.sizeof(S)] + [getattr(S, name).offset for name in FIELDS]
    assert got[6:] == [56, 188, 84, 168, 184]
    assert C.sizeof(art.ArtAovBuffers) == 56 and C.sizeof(art.ArtTemporalParams) == 188 and C.sizeof(art.ArtTemporalCamera) == 84


def test_refused_with_a_message_before_anything_is_launched(art):
    """In a process of its own, where no scene was ever uploaded: the refusals that need no scene and no device come first, under the
    new calls' own names; with motion3f NULL the calls are the old ones and say so."""
    code = ("import sys, ctypes as C; sys.path.insert(0, %r); import __graft_entry__ as g; art = g.load_package(); L = art.load_library()\n"
            "p = art.Backend.pass_params(); buf = art.ArtAovBuffers(); src = art.ArtMotionSource(); m = 0x1000      # never dereferenced\n"
            "for args in ((C.byref(p), None, None, m), (None, None, C.byref(src), m), (C.byref(p), None, C.byref(src), m), (C.byref(p), None, C.byref(src), None),\n"
            "             (C.byref(p), C.byref(buf), None, None)):\n"
            "    print(L.art_render_aovs_motion_device(*args, None), L.art_last_error().decode())\n"
            "t = art.ArtTemporalParams()\n"
            "print(L.art_temporal_motion_device(C.byref(t), None, None, None, None, None, m, None, None, None, None, None, None), L.art_last_error().decode())\n"
            "print(L.art_temporal_motion_device(C.byref(t), None, None, None, None, None, None, None, None, None, None, None, None), L.art_last_error().decode())\n") % art.ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300).stdout.splitlines()
    assert len(out) == 7 and all(line.split()[0] != "0" for line in out), out
    assert "art_render_aovs_motion_device: motion3f needs an ArtMotionSource" in out[0]
    assert "art_render_aovs_motion_device: null ArtPassParams" in out[1]
    assert "art_render_aovs_motion_device: no scene uploaded" in out[2]
    assert "art_render_aovs_device: null ArtAovBuffers" in out[3]
    assert "art_render_aovs_device: no plane is wanted" in out[4]
    assert "art_temporal_motion_device: null color3f" in out[5]
    assert "art_temporal_device: null color3f" in out[6]


def test_the_python_wrapper_checks_its_tensors_before_any_call(art):
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    with pytest.raises(ValueError, match="nope"):
        be.render_aovs_torch_motion(art.Backend.pass_params(), want=("nope",))
    torch = pytest.importorskip("torch")
    pos = torch.zeros((5, 3))
    with pytest.raises(art.ArtError, match="GPU tensor"):
        be.render_aovs_torch_motion(art.Backend.pass_params(), cur_pos=pos, prev_pos=pos)
    with pytest.raises(art.ArtError, match="dtype"):
        be.render_aovs_torch_motion(art.Backend.pass_params(), prev_matrices=torch.zeros((2, 12), dtype=torch.float64))
    with pytest.raises(art.ArtError, match=r"shape must be \[n, 12\]"):
        be.render_aovs_torch_motion(art.Backend.pass_params(), prev_matrices=torch.zeros((2, 11)))
