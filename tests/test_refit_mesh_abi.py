"""Deforming an instanced mesh without a GPU: art_refit_mesh_device / art_get_mesh_refit_info are declared and exported, ArtMeshRefitInfo
matches the header, a refit without a scene is refused before anything touches a device, Backend.refit_mesh_torch checks its tensors
on the host, and the Ada spec binds both calls."""
import ctypes as C
import os
import re

import pytest


def test_mesh_refit_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    for name in ("art_refit_mesh_device", "art_get_mesh_refit_info"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in art.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    assert re.search(r"int\s+art_refit_mesh_device\(int32_t mesh, const float\* pos3f, const float\* nrm3f, int64_t nverts, void\* hip_stream\);", hdr)
    assert re.search(r"int\s+art_get_mesh_refit_info\(ArtMeshRefitInfo\* out\);", hdr)
    assert re.search(r"typedef struct ArtMeshRefitInfo \{ uint64_t refits; double refit_ms; double plan_ms; uint64_t bad_vertices; uint64_t repads; \} ArtMeshRefitInfo;", hdr)
    I = art.ArtMeshRefitInfo
    assert C.sizeof(I) == 40
    assert (I.refits.offset, I.refit_ms.offset, I.plan_ms.offset, I.bad_vertices.offset, I.repads.offset) == (0, 8, 16, 24, 32)
    assert [t for _, t in I._fields_] == [C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_uint64]
    assert L.art_refit_mesh_device.argtypes == [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]


def test_mesh_refit_without_a_scene_is_refused(art):
    L = art.load_library()
    assert L.art_refit_mesh_device(0, None, None, 0, None) != 0
    assert "art_refit_mesh_device: no scene uploaded" in L.art_last_error().decode()
    assert L.art_get_mesh_refit_info(None) != 0
    assert "null ArtMeshRefitInfo" in L.art_last_error().decode()


def test_refit_mesh_torch_checks_dtype_and_shape_on_the_host(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)      # (Backend() itself needs a GPU: art_init fails first)
    be.lib = art.load_library()
    pos = torch.zeros((7, 3), dtype=torch.float32)
    with pytest.raises(art.ArtError, match="float32"):
        be.refit_mesh_torch(0, pos.double())
    with pytest.raises(art.ArtError, match="float32"):
        be.refit_mesh_torch(0, pos, pos.half())
    with pytest.raises(art.ArtError, match="shape"):
        be.refit_mesh_torch(0, torch.zeros((7, 4)))
    with pytest.raises(art.ArtError, match="shape"):
        be.refit_mesh_torch(0, pos, torch.zeros((6, 3)))
    with pytest.raises(art.ArtError, match=r"\[nverts, 3\]"):
        be.refit_mesh_torch(0, torch.zeros(21))
    with pytest.raises(art.ArtError, match=r"\[nverts, 3\]"):
        be.refit_mesh_torch(0, [[0.0, 0.0, 0.0]])
    with pytest.raises(art.ArtError, match="torch tensor"):
        be.refit_mesh_torch(0, pos, [[0.0, 0.0, 0.0]] * 7)


def test_the_ada_spec_binds_both_calls(art):
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    for name in ("art_refit_mesh_device", "art_get_mesh_refit_info"):
        assert re.search(r"function %s\b" % name, ads), name
        assert re.search(r'pragma Import \(C, %s, "%s"\);' % (name, name), ads), name
    rec = re.search(r"type Art_Mesh_Refit_Info is record(.*?)end record;", ads, flags=re.S)
    assert rec and re.findall(r"^\s*(\w+)\s*:", re.sub(r"--.*", "", rec.group(1)), flags=re.M) == ["refits", "refit_ms", "plan_ms", "bad_vertices", "repads"]
