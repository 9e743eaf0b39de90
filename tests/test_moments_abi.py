"""art_bind_moments without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in Ada; the
Python binding refuses bad tensors with no library call."""
import os
import re
import subprocess


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_bind_moments\(void\* device_moments_rowmajor\);", hdr)
    assert "art_bind_moments" in art.EXPORTED_SYMBOLS
    assert getattr(art.load_library(), "art_bind_moments") is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert re.search(r"\bT art_bind_moments$", out, flags=re.M)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert 'pragma Import (C, art_bind_moments, "art_bind_moments");' in ads


def test_the_kernels_exist_next_to_the_old_ones(art):
    """k_accumulate_moments is a kernel of its own: k_accumulate is still there for the passes without moments"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", "-C", art.LIB_PATH], text=True)
    assert re.search(r"art::k_accumulate\(", out) and re.search(r"art::k_accumulate_moments\(", out)


def test_python_refuses_bad_tensors_before_any_call(art):
    """bind_moments checks its tensor on the host with bind_accum's messages, and resize() refuses a frame a held tensor is too small for:
    no library call is made for either"""
    import pytest
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    be._accum_tensor = be._moments_tensor = None
    for bad, msg in (([[1.0, 2.0]], "None, an integer device address or a torch tensor"), ("moments", "torch tensor is required"),
                     (torch.zeros(8), "must be a GPU tensor"), (torch.zeros(8, dtype=torch.float64), "GPU tensor|dtype")):
        with pytest.raises(art.ArtError, match="bind_moments: .*(%s)" % msg):
            be.bind_moments(bad)
        assert be._moments_tensor is None

    class Held:                                           # what resize() reads of a held tensor
        def __init__(self, n):
            self.n = n

        def numel(self):
            return self.n
    be._moments_tensor = Held(2 * 4 * 4)
    with pytest.raises(art.ArtError, match="bound moments tensor"):
        be.resize(5, 4)
    be._moments_tensor, be._accum_tensor = None, Held(3 * 4 * 4)
    with pytest.raises(art.ArtError, match="bound accum tensor"):
        be.resize(5, 4)
