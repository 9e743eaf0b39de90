"""Moving instances without a GPU: art_move_instances_device / art_get_move_info are declared and exported, ArtMoveInfo matches the
header, a move without a scene is refused before anything touches a device, and Backend.move_instances_torch checks its tensor on
the host."""
import ctypes as C
import os
import re

import pytest


def test_move_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    for name in ("art_move_instances_device", "art_get_move_info"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in art.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    assert re.search(r"int\s+art_move_instances_device\(const float\* m12f, int64_t n_instances, void\* hip_stream\);", hdr)
    assert re.search(r"typedef struct ArtMoveInfo \{ uint64_t moves; double move_ms; double plan_ms; uint64_t bad_matrices; uint64_t repads; \} ArtMoveInfo;", hdr)
    I = art.ArtMoveInfo
    assert C.sizeof(I) == 40
    assert (I.moves.offset, I.move_ms.offset, I.plan_ms.offset, I.bad_matrices.offset, I.repads.offset) == (0, 8, 16, 24, 32)


def test_move_without_a_scene_is_refused(art):
    L = art.load_library()
    assert L.art_move_instances_device(None, 0, None) != 0
    assert "no scene uploaded" in L.art_last_error().decode()
    assert L.art_get_move_info(None) != 0


def test_move_instances_torch_checks_dtype_and_shape_on_the_host(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)      # (Backend() itself needs a GPU: art_init fails first)
    be.lib = art.load_library()
    m = torch.zeros((5, 3, 4), dtype=torch.float32)
    with pytest.raises(art.ArtError, match="float32"):
        be.move_instances_torch(m.double())
    with pytest.raises(art.ArtError, match="shape"):
        be.move_instances_torch(torch.zeros((5, 4, 3)))
    with pytest.raises(art.ArtError, match="shape"):
        be.move_instances_torch(torch.zeros((5, 16)))
    with pytest.raises(art.ArtError, match="shape"):
        be.move_instances_torch(torch.zeros(60))
    with pytest.raises(art.ArtError, match="torch tensor"):
        be.move_instances_torch([[0.0] * 12])
