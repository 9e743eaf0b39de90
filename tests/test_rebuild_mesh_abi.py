"""A new tree for one mesh of an instanced scene on the GPU and its cost figure, without a GPU: art_rebuild_mesh_tree_device,
art_get_mesh_rebuild_info and art_get_mesh_tree_cost are declared and exported, the struct matches the header as compiled, and the
calls fail cleanly without a scene or a device."""
import ctypes as C
import os
import re
import subprocess

NAMES = ("art_rebuild_mesh_tree_device", "art_get_mesh_rebuild_info", "art_get_mesh_tree_cost")


def test_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in art.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    assert re.search(r"int\s+art_rebuild_mesh_tree_device\(int32_t mesh, void\* hip_stream\);", hdr)
    assert re.search(r"typedef struct ArtMeshRebuildInfo \{ uint64_t rebuilds; double gather_ms, build_ms, host_ms; \} ArtMeshRebuildInfo;", hdr)
    assert re.search(r"int\s+art_get_mesh_rebuild_info\(ArtMeshRebuildInfo\* out\);", hdr)
    assert re.search(r"int\s+art_get_mesh_tree_cost\(int32_t mesh, ArtTreeCost\* out\);", hdr)
    I = art.ArtMeshRebuildInfo
    assert C.sizeof(I) == 32 and I.rebuilds.offset == 0 and I.gather_ms.offset == 8 and I.build_ms.offset == 16 and I.host_ms.offset == 24
    # the structs next to it are left as they were
    assert C.sizeof(art.ArtTreeCost) == 32 and C.sizeof(art.ArtInstanceRebuildInfo) == 32 and C.sizeof(art.ArtMeshRefitInfo) == 40
    ads = open(os.path.join(art.ROOT, "ada-ray-tracer_amd", "ada", "art_hip.ads")).read()
    for name in NAMES:
        assert 'pragma Import (C, %s, "%s");' % (name, name) in ads, name


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    """sizeof / offsetof from a C compiler reading include/art_hip.h against the ctypes mirror."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ArtMeshRebuildInfo), '
                   'offsetof(ArtMeshRebuildInfo, rebuilds), offsetof(ArtMeshRebuildInfo, gather_ms), offsetof(ArtMeshRebuildInfo, build_ms), '
                   'offsetof(ArtMeshRebuildInfo, host_ms)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    I = art.ArtMeshRebuildInfo
    assert got == [C.sizeof(I), I.rebuilds.offset, I.gather_ms.offset, I.build_ms.offset, I.host_ms.offset]


def test_without_a_scene_the_calls_are_refused(art):
    L = art.load_library()
    assert L.art_rebuild_mesh_tree_device(0, None) != 0
    assert "art_rebuild_mesh_tree_device: no scene uploaded" in L.art_last_error().decode()
    tc = art.ArtTreeCost()
    assert L.art_get_mesh_tree_cost(0, C.byref(tc)) != 0
    assert "art_get_mesh_tree_cost: no scene uploaded" in L.art_last_error().decode()
    assert L.art_get_mesh_tree_cost(0, None) != 0
    assert L.art_get_mesh_rebuild_info(None) != 0
    ri = art.ArtMeshRebuildInfo()
    assert L.art_get_mesh_rebuild_info(C.byref(ri)) == 0 and ri.rebuilds == 0 and ri.host_ms == 0.0      # (a counter: needs no scene)


def test_the_backend_methods_exist_and_fail_cleanly_without_a_scene(art):
    be = art.Backend.__new__(art.Backend)      # (Backend() itself needs a GPU: art_init fails first)
    be.lib = art.load_library()
    for call in (lambda: be.rebuild_mesh(0), lambda: be.mesh_tree_cost(0)):
        try:
            call()
        except art.ArtError as e:
            assert "no scene uploaded" in str(e)
        else:
            raise AssertionError("accepted without a scene")
    assert be.mesh_rebuild_info().rebuilds == 0
