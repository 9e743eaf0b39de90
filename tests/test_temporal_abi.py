"""art_temporal_device, art_temporal_history_bytes and art_denoise_svgf_var_device without a GPU: declared in the header, exported by the
library, listed in EXPORTED_SYMBOLS and bound in Ada; the structs match the header as compiled; what can be refused without a device is."""
import ctypes as C
import os
import re
import subprocess

import pytest

NAMES = ("art_temporal_device", "art_temporal_history_bytes", "art_denoise_svgf_var_device")
CAM_FIELDS = ("cam_pos", "cam_matrix", "width", "height")
FIELDS = ("cur", "prev", "n_colours", "max_history", "scale", "depth_tol", "normal_min")


def test_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_temporal_device\(const ArtTemporalParams\* p, const float\* color3f, const float\* moments2f, const float\* normal3f, const float\* depth,\s*"
                     r"const int32_t\* id, const void\* hist_in, void\* hist_out, float\* out3f, float\* variance_out, float\* length_out,\s*void\* hip_stream\);", hdr)
    assert re.search(r"int64_t art_temporal_history_bytes\(int32_t width, int32_t height\);", hdr)
    assert re.search(r"int\s+art_denoise_svgf_var_device\(const ArtSvgfParams\* p, const float\* color3f, const float\* variance1f, const float\* albedo3f,\s*"
                     r"const float\* normal3f, const float\* depth, float\* out3f, float\* variance_out, void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    for name in NAMES:
        assert name in art.EXPORTED_SYMBOLS and getattr(art.load_library(), name) is not None
        assert re.search(r"\bT %s$" % name, out, flags=re.M)
        assert 'pragma Import (C, %s, "%s");' % (name, name) in ads
    assert re.search(r"\bT art_denoise_svgf_device$", out, flags=re.M)


def test_structs_match_the_header_as_compiled(art, tmp_path):
    import temporal_ref
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtTemporalCamera));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtTemporalCamera, %s));\n' % n for n in CAM_FIELDS)
                   + '  printf(" %zu", sizeof(ArtTemporalParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtTemporalParams, %s));\n' % n for n in FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [84, 0, 12, 76, 80, 188, 0, 84, 168, 172, 176, 180, 184]
    assert got == want
    for cam, par in ((art.ArtTemporalCamera, art.ArtTemporalParams), (temporal_ref.Camera, temporal_ref.Params)):
        assert [C.sizeof(cam)] + [getattr(cam, n).offset for n in CAM_FIELDS] + [C.sizeof(par)] + [getattr(par, n).offset for n in FIELDS] == want


def test_history_bytes(art):
    L = art.load_library()
    assert L.art_temporal_history_bytes(7, 3) == 48 * 21 and L.art_temporal_history_bytes(1 << 14, 1 << 14) == 48 << 28
    for w, h in ((0, 4), (4, -1), (1 << 15, 1 << 14)):
        assert L.art_temporal_history_bytes(w, h) == 0


def test_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call)"""
    L = art.load_library()
    one = C.c_void_p(16)                    # never dereferenced: every call below is refused on its parameters
    eye = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]

    def params(**kw):
        p = art.ArtTemporalParams()
        for cam in (p.cur, p.prev):
            cam.cam_matrix = (C.c_float * 16)(*eye); cam.width = 4; cam.height = 4
        p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = 2, 16, 1.0, 0.05, 0.9
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(p, text, color=one, mom=one, hin=None, hout=one):
        rc = L.art_temporal_device(C.byref(p) if p is not None else None, color, mom, None, None, None, hin, hout, None, None, None, None)
        assert rc != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())
    refused(None, "null ArtTemporalParams")
    refused(params(), "null color3f, moments2f or hist_out", color=None)
    refused(params(), "null color3f, moments2f or hist_out", mom=None)
    refused(params(), "null color3f, moments2f or hist_out", hout=None)
    refused(params(n_colours=0), "n_colours")
    refused(params(max_history=1), "max_history")
    refused(params(max_history=(1 << 24) + 1), "max_history")
    refused(params(scale=float("inf")), "scale")
    refused(params(depth_tol=float("nan")), "depth_tol")
    refused(params(normal_min=float("nan")), "depth_tol or normal_min")
    p = params(); p.cur.width = 0
    refused(p, "cur: width")
    p = params(); p.prev.height = 0
    refused(p, "prev: width", hin=one)
    p = params(); p.cur.cam_matrix[7] = 0.5
    refused(p, "cur: the camera is refused")
    p = params(); p.cur.cam_pos[1] = float("nan")
    refused(p, "cur: the camera is refused")
    p = params(); p.prev.cam_matrix[0] = 0.0
    refused(p, "prev: the camera is refused", hin=one)
    s = art.ArtSvgfParams(4, 4, 2, 0, 7, 0, 1.0, 2.0, 1.0)
    assert L.art_denoise_svgf_var_device(C.byref(s), one, None, None, None, None, one, None, None) != 0 and "null variance1f" in L.art_last_error().decode()
    assert L.art_denoise_svgf_var_device(None, one, one, None, None, None, one, None, None) != 0 and "art_denoise_svgf_var_device: null ArtSvgfParams" in L.art_last_error().decode()
    s.iterations = 9
    assert L.art_denoise_svgf_var_device(C.byref(s), one, one, None, None, None, one, None, None) != 0 and "iterations" in L.art_last_error().decode()


def test_python_refuses_bad_tensors_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    cam = ([0, 0, 0], [1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    col, mom = torch.zeros(4, 4, 3), torch.zeros(4, 4, 2)
    with pytest.raises(art.ArtError, match="cur: a dict"):
        be.temporal_torch(col, None, cam, None, 2)
    with pytest.raises(art.ArtError, match="color: a torch tensor"):
        be.temporal_torch(dict(moments=mom), None, cam, None, 2)
    with pytest.raises(art.ArtError, match="color: shape"):
        be.temporal_torch(dict(color=torch.zeros(4, 4), moments=mom), None, cam, None, 2)
    with pytest.raises(art.ArtError, match="moments: a torch tensor"):
        be.temporal_torch(dict(color=col), None, cam, None, 2)
    with pytest.raises(art.ArtError, match="moments: shape"):
        be.temporal_torch(dict(color=col, moments=torch.zeros(4, 4)), None, cam, None, 2)
    with pytest.raises(art.ArtError, match="depth: shape"):
        be.temporal_torch(dict(color=col, moments=mom, depth=torch.zeros(4, 4, 1)), None, cam, None, 2)
    with pytest.raises(art.ArtError, match="prim_index: dtype"):
        be.temporal_torch(dict(color=col, moments=mom, prim_index=torch.zeros(4, 4)), None, cam, None, 2)
    with pytest.raises(art.ArtError, match="history: shape"):
        be.temporal_torch(dict(color=col, moments=mom), torch.zeros(4, 4, 12), cam, cam, 2)
    with pytest.raises(art.ArtError, match="contiguous"):
        be.temporal_torch(dict(color=torch.zeros(4, 3, 4).permute(0, 2, 1), moments=mom), None, cam, None, 2)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        be.temporal_torch(dict(color=col, moments=mom), None, cam, None, 2)
    with pytest.raises(art.ArtError, match="cam_prev: a history needs"):
        be.temporal_torch(dict(color=col, moments=mom), torch.zeros(3, 4, 4, 4), cam, None, 2)
    with pytest.raises(art.ArtError, match="cam_cur: a camera is"):
        be.temporal_torch(dict(color=col, moments=mom), None, [0, 0, 0], None, 2)
    with pytest.raises(art.ArtError, match="not both"):
        be.denoise_svgf_torch(col, n_colours=4, variance=torch.zeros(4, 4))
    with pytest.raises(art.ArtError, match="variance: shape"):
        be.denoise_svgf_torch(col, variance=torch.zeros(4, 4, 1))
    with pytest.raises(art.ArtError, match="not both"):
        be.denoise_svgf_torch(col, mom, 2, variance=torch.zeros(4, 4))
    with pytest.raises(art.ArtError, match="GPU tensor"):
        be.denoise_svgf_torch(col, variance=torch.zeros(4, 4))
