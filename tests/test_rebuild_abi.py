"""A new tree on the GPU and the tree-cost figure, without a GPU: art_rebuild_device / art_get_rebuild_info / art_get_tree_cost are
declared and exported, the two structs match the header as compiled, the calls fail cleanly without a scene or a device, and
Backend.rebuild_torch checks its tensors on the host like refit_torch."""
import ctypes as C
import os
import re
import subprocess

import pytest


def test_rebuild_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    for name in ("art_rebuild_device", "art_get_rebuild_info", "art_get_tree_cost"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in art.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    assert re.search(r"typedef struct ArtRebuildInfo \{ uint64_t rebuilds; double gather_ms; double build_ms; double host_ms; \} ArtRebuildInfo;", hdr)
    assert re.search(r"typedef struct ArtTreeCost \{ double root_area, node_visits, leaf_visits, tri_tests; \} ArtTreeCost;", hdr)
    assert re.search(r"int\s+art_rebuild_device\(const float\* pos3f, const float\* nrm3f, int64_t nverts, void\* hip_stream\);", hdr)
    assert C.sizeof(art.ArtRebuildInfo) == 32 and art.ArtRebuildInfo.gather_ms.offset == 8 and art.ArtRebuildInfo.host_ms.offset == 24
    assert C.sizeof(art.ArtTreeCost) == 32 and art.ArtTreeCost.node_visits.offset == 8 and art.ArtTreeCost.tri_tests.offset == 24
    # ArtRefitInfo is left as it was
    assert C.sizeof(art.ArtRefitInfo) == 32 and art.ArtRefitInfo.bad_vertices.offset == 24


def test_structs_match_the_header_as_compiled(art, tmp_path):
    """sizeof / offsetof from a C compiler reading include/art_hip.h against the ctypes mirrors."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ArtRebuildInfo), '
                   'offsetof(ArtRebuildInfo, build_ms), offsetof(ArtRebuildInfo, host_ms), sizeof(ArtTreeCost), offsetof(ArtTreeCost, leaf_visits), '
                   'offsetof(ArtTreeCost, tri_tests)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(art.ArtRebuildInfo), art.ArtRebuildInfo.build_ms.offset, art.ArtRebuildInfo.host_ms.offset,
                   C.sizeof(art.ArtTreeCost), art.ArtTreeCost.leaf_visits.offset, art.ArtTreeCost.tri_tests.offset]


def test_rebuild_and_tree_cost_without_a_scene_are_refused(art):
    L = art.load_library()
    assert L.art_rebuild_device(None, None, 0, None) != 0
    assert "art_rebuild_device: no scene uploaded" in L.art_last_error().decode()
    tc = art.ArtTreeCost()
    assert L.art_get_tree_cost(C.byref(tc)) != 0
    assert "art_get_tree_cost: no scene uploaded" in L.art_last_error().decode()
    assert L.art_get_tree_cost(None) != 0
    assert L.art_get_rebuild_info(None) != 0
    ri = art.ArtRebuildInfo()
    assert L.art_get_rebuild_info(C.byref(ri)) == 0 and ri.rebuilds == 0 and ri.host_ms == 0.0      # (a counter: needs no scene)


def test_rebuild_torch_checks_dtype_and_shape_on_the_host(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)      # (Backend() itself needs a GPU: art_init fails first)
    be.lib = art.load_library()
    p = torch.zeros((5, 3), dtype=torch.float32)
    with pytest.raises(art.ArtError, match="float32"):
        be.rebuild_torch(p.double())
    with pytest.raises(art.ArtError, match="shape"):
        be.rebuild_torch(torch.zeros((5, 4)))
    with pytest.raises(art.ArtError, match="shape"):
        be.rebuild_torch(p, torch.zeros((4, 3)))
    with pytest.raises(art.ArtError, match=r"\[nverts, 3\]"):
        be.rebuild_torch(torch.zeros(15))
    if not torch.cuda.is_available():
        with pytest.raises(art.ArtError, match="no HIP device"):       # past the host checks: no device, a clean message
            be.rebuild_torch(p)
        with pytest.raises(art.ArtError):
            be.tree_cost()
