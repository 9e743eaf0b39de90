"""A new instance tree on the GPU and its cost figure, without a GPU: art_rebuild_instance_tree_device, art_get_instance_rebuild_info and
art_get_instance_tree_cost are declared and exported, the structs match the header as compiled, and the calls fail cleanly without a
scene or a device."""
import ctypes as C
import os
import re
import subprocess

NAMES = ("art_rebuild_instance_tree_device", "art_get_instance_rebuild_info", "art_get_instance_tree_cost")


def test_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in art.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    assert re.search(r"int\s+art_rebuild_instance_tree_device\(void\* hip_stream\);", hdr)
    assert re.search(r"typedef struct ArtInstanceRebuildInfo \{ uint64_t rebuilds; double gather_ms, build_ms, host_ms; \} ArtInstanceRebuildInfo;", hdr)
    assert re.search(r"int\s+art_get_instance_rebuild_info\(ArtInstanceRebuildInfo\* out\);", hdr)
    assert re.search(r"int\s+art_get_instance_tree_cost\(ArtTreeCost\* out\);", hdr)
    I = art.ArtInstanceRebuildInfo
    assert C.sizeof(I) == 32 and I.rebuilds.offset == 0 and I.gather_ms.offset == 8 and I.build_ms.offset == 16 and I.host_ms.offset == 24
    # the structs next to it are left as they were
    assert C.sizeof(art.ArtTreeCost) == 32 and C.sizeof(art.ArtRebuildInfo) == 32 and C.sizeof(art.ArtMoveInfo) == 40


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    """sizeof / offsetof from a C compiler reading include/art_hip.h against the ctypes mirror."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ArtInstanceRebuildInfo), '
                   'offsetof(ArtInstanceRebuildInfo, rebuilds), offsetof(ArtInstanceRebuildInfo, gather_ms), offsetof(ArtInstanceRebuildInfo, build_ms), '
                   'offsetof(ArtInstanceRebuildInfo, host_ms)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    I = art.ArtInstanceRebuildInfo
    assert got == [C.sizeof(I), I.rebuilds.offset, I.gather_ms.offset, I.build_ms.offset, I.host_ms.offset]


def test_without_a_scene_the_calls_are_refused(art):
    L = art.load_library()
    assert L.art_rebuild_instance_tree_device(None) != 0
    assert "art_rebuild_instance_tree_device: no scene uploaded" in L.art_last_error().decode()
    tc = art.ArtTreeCost()
    assert L.art_get_instance_tree_cost(C.byref(tc)) != 0
    assert "art_get_instance_tree_cost: no scene uploaded" in L.art_last_error().decode()
    assert L.art_get_instance_tree_cost(None) != 0
    assert L.art_get_instance_rebuild_info(None) != 0
    ri = art.ArtInstanceRebuildInfo()
    assert L.art_get_instance_rebuild_info(C.byref(ri)) == 0 and ri.rebuilds == 0 and ri.host_ms == 0.0      # (a counter: needs no scene)


def test_the_backend_methods_exist_and_fail_cleanly_without_a_scene(art):
    be = art.Backend.__new__(art.Backend)      # (Backend() itself needs a GPU: art_init fails first)
    be.lib = art.load_library()
    for call in (be.rebuild_instances, be.instance_tree_cost):
        try:
            call()
        except art.ArtError as e:
            assert "no scene uploaded" in str(e)
        else:
            raise AssertionError("accepted without a scene")
    assert be.instance_rebuild_info().rebuilds == 0
