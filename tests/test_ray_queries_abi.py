"""Device-resident ray queries without a GPU: both entry points are declared and exported, the torch methods validate their inputs
on the host, and without a device they fail with the library's "no HIP device" error instead of falling back to a CPU path."""
import ctypes as C
import os
import re

import pytest


def test_query_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    for name in ("art_trace_rays_device", "art_occluded_rays_device"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in art.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None


def _hostless_backend(art):
    be = art.Backend.__new__(art.Backend)     # (Backend() itself needs a GPU: art_init fails first)
    be.lib = art.load_library()
    return be


def _has_gpu(art):
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; a = g.load_package()\n"
            "try:\n    a.Backend(0); print('HAS_GPU')\nexcept a.ArtError as e:\n    print('ERR', e)\n") % art.ROOT
    return "HAS_GPU" in subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300).stdout


def test_torch_queries_fail_without_a_device(art):
    torch = pytest.importorskip("torch")
    if _has_gpu(art):
        pytest.skip("a GPU is present")
    be = _hostless_backend(art)
    o = torch.zeros((4, 3), dtype=torch.float32); d = torch.ones((4, 3), dtype=torch.float32)
    for call in (lambda: be.trace_rays_torch(o, d), lambda: be.occluded_torch(o, d, tfar=torch.ones(4))):
        with pytest.raises(art.ArtError, match="no HIP device"):
            call()
    L = art.load_library()
    assert L.art_occluded_rays_device(None, None, None, None, 0, None, None) != 0
    assert "no HIP device" in L.art_last_error().decode()


def test_torch_queries_check_dtype_and_shape_on_the_host(art):
    torch = pytest.importorskip("torch")
    be = _hostless_backend(art)
    o = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(art.ArtError, match="float32"):
        be.trace_rays_torch(o.double(), o)
    with pytest.raises(art.ArtError, match="shape"):
        be.trace_rays_torch(o, torch.zeros((5, 3)))
    with pytest.raises(art.ArtError, match="shape"):
        be.occluded_torch(o, o, tfar=torch.ones(3))
    with pytest.raises(art.ArtError, match="shape"):
        be.trace_rays_torch(torch.zeros((4, 4)), torch.zeros((4, 4)))


def test_package_import_stays_torch_free(art):
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; g.load_package(); print('torch' in sys.modules)") % art.ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300).stdout.strip()
    assert out == "False"
