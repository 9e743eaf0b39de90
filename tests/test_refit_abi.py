"""Moving geometry without a GPU: art_refit_device / art_get_refit_info are declared and exported, ArtRefitInfo matches the header,
a refit without a scene is refused before anything touches a device, and Backend.refit_torch checks its tensors on the host."""
import ctypes as C
import os
import re

import pytest


def test_refit_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    for name in ("art_refit_device", "art_get_refit_info"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in art.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    assert re.search(r"typedef struct ArtRefitInfo \{ uint64_t refits; double refit_ms; double plan_ms; uint64_t bad_vertices; \} ArtRefitInfo;", hdr)
    assert C.sizeof(art.ArtRefitInfo) == 32 and art.ArtRefitInfo.plan_ms.offset == 16 and art.ArtRefitInfo.bad_vertices.offset == 24


def test_refit_without_a_scene_is_refused(art):
    L = art.load_library()
    assert L.art_refit_device(None, None, 0, None) != 0
    assert "no scene uploaded" in L.art_last_error().decode()
    assert L.art_get_refit_info(None) != 0


def test_refit_torch_checks_dtype_and_shape_on_the_host(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)      # (Backend() itself needs a GPU: art_init fails first)
    be.lib = art.load_library()
    p = torch.zeros((5, 3), dtype=torch.float32)
    with pytest.raises(art.ArtError, match="float32"):
        be.refit_torch(p.double())
    with pytest.raises(art.ArtError, match="shape"):
        be.refit_torch(torch.zeros((5, 4)))
    with pytest.raises(art.ArtError, match="shape"):
        be.refit_torch(p, torch.zeros((4, 3)))
    with pytest.raises(art.ArtError, match=r"\[nverts, 3\]"):
        be.refit_torch(torch.zeros(15))
