"""art_denoise_device without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in Ada;
ArtDenoiseParams matches the header as compiled."""
import ctypes as C
import os
import re
import subprocess

FIELDS = ("width", "height", "iterations", "demodulate", "normal_log2", "variant", "scale", "sigma_color", "sigma_depth")


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_denoise_device\(const ArtDenoiseParams\* p, const float\* color3f,\s*const float\* albedo3f, const float\* normal3f, "
                     r"const float\* depth,\s*float\* out3f, void\* hip_stream\);", hdr)
    assert "art_denoise_device" in art.EXPORTED_SYMBOLS
    assert getattr(art.load_library(), "art_denoise_device") is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert re.search(r"\bT art_denoise_device$", out, flags=re.M)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert 'pragma Import (C, art_denoise_device, "art_denoise_device");' in ads


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    """sizeof / offsetof from a C compiler reading include/art_hip.h against the ctypes mirrors (the package's and the test helper's)"""
    import denoise_ref
    B = art.ArtDenoiseParams
    assert [name for name, _ in B._fields_] == list(FIELDS) == [name for name, _ in denoise_ref.Params._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtDenoiseParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtDenoiseParams, %s));\n' % name for name in FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(B)] + [getattr(B, name).offset for name in FIELDS] == [36] + list(range(0, 36, 4))
    assert C.sizeof(denoise_ref.Params) == 36
    assert C.sizeof(art.ArtAovBuffers) == 56 and C.sizeof(art.ArtPassParams) == 48      # the structs next to it are left as they were


def test_python_refuses_bad_tensors_before_any_call(art):
    """denoise_torch checks its tensors on the host: no library call is made for a refused one"""
    import pytest
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    with pytest.raises(art.ArtError, match="torch tensor"):
        be.denoise_torch([[1.0, 2.0, 3.0]])
    with pytest.raises(art.ArtError, match="shape"):
        be.denoise_torch(torch.zeros(4, 4))
    with pytest.raises(art.ArtError, match="GPU tensor"):
        be.denoise_torch(torch.zeros(4, 4, 3))
    with pytest.raises(art.ArtError, match="dtype"):
        be.denoise_torch(torch.zeros(4, 4, 3, dtype=torch.float64))
    with pytest.raises(art.ArtError, match="contiguous"):
        be.denoise_torch(torch.zeros(4, 3, 4).permute(0, 2, 1))
    with pytest.raises(TypeError, match="nope"):
        be.denoise_torch(torch.zeros(4, 4, 3), nope=None)
