"""art_set_camera without a GPU: declared in the header, exported, listed in EXPORTED_SYMBOLS and bound in Ada; refused without a scene."""
import ctypes as C
import os
import re
import subprocess


def test_symbol_declared_exported_and_refused_without_a_scene(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_set_camera\(const float cam_pos\[3\], const float cam_matrix\[16\]\);", hdr)
    assert "art_set_camera" in art.EXPORTED_SYMBOLS and hasattr(art.Backend, "set_camera")
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert re.search(r"\bT art_set_camera$", out, flags=re.M)
    assert 'pragma Import (C, art_set_camera, "art_set_camera");' in open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    L = art.load_library()
    pos, m = (C.c_float * 3)(0, 0, 0), (C.c_float * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    assert L.art_set_camera(C.byref(pos), C.byref(m)) != 0 and "art_set_camera: no scene uploaded" in L.art_last_error().decode()
