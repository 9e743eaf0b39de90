"""art_denoise_svgf_device without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in Ada;
ArtSvgfParams matches the header as compiled, and ArtDenoiseParams is what it was."""
import ctypes as C
import os
import re
import subprocess

FIELDS = ("width", "height", "iterations", "demodulate", "normal_log2", "n_colours", "scale", "sigma_color", "sigma_depth")
OLD_FIELDS = ("width", "height", "iterations", "demodulate", "normal_log2", "variant", "scale", "sigma_color", "sigma_depth")


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_denoise_svgf_device\(const ArtSvgfParams\* p, const float\* color3f, const float\* moments2f, const float\* albedo3f,\s*"
                     r"const float\* normal3f, const float\* depth, float\* out3f, float\* variance_out, void\* hip_stream\);", hdr)
    assert "art_denoise_svgf_device" in art.EXPORTED_SYMBOLS
    assert getattr(art.load_library(), "art_denoise_svgf_device") is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert re.search(r"\bT art_denoise_svgf_device$", out, flags=re.M)
    assert re.search(r"\bT art_denoise_device$", out, flags=re.M)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert 'pragma Import (C, art_denoise_svgf_device, "art_denoise_svgf_device");' in ads


def test_structs_match_the_header_as_compiled(art, tmp_path):
    """sizeof / offsetof from a C compiler reading include/art_hip.h against the ctypes mirrors (the package's and the test helper's)"""
    import svgf_ref
    B = art.ArtSvgfParams
    assert [name for name, _ in B._fields_] == list(FIELDS) == [name for name, _ in svgf_ref.Params._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtSvgfParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtSvgfParams, %s));\n' % name for name in FIELDS)
                   + '  printf(" %zu", sizeof(ArtDenoiseParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtDenoiseParams, %s));\n' % name for name in OLD_FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [36] + list(range(0, 36, 4))
    assert got[:10] == [C.sizeof(B)] + [getattr(B, name).offset for name in FIELDS] == want
    assert got[10:] == [C.sizeof(art.ArtDenoiseParams)] + [getattr(art.ArtDenoiseParams, name).offset for name in OLD_FIELDS] == want
    assert C.sizeof(svgf_ref.Params) == 36


def test_python_refuses_bad_tensors_before_any_call(art):
    """denoise_svgf_torch checks its tensors on the host: no library call is made for a refused one"""
    import pytest
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    m = torch.zeros(4, 4, 2)
    with pytest.raises(art.ArtError, match="color: a torch tensor"):
        be.denoise_svgf_torch([[1.0, 2.0, 3.0]], m, 2)
    with pytest.raises(art.ArtError, match="color: shape"):
        be.denoise_svgf_torch(torch.zeros(4, 4), m, 2)
    with pytest.raises(art.ArtError, match="moments: a torch tensor"):
        be.denoise_svgf_torch(torch.zeros(4, 4, 3), None, 2)
    with pytest.raises(art.ArtError, match="moments: dtype"):
        be.denoise_svgf_torch(torch.zeros(4, 4, 3), m.double(), 2)
    with pytest.raises(art.ArtError, match="moments: shape"):
        be.denoise_svgf_torch(torch.zeros(4, 4, 3), torch.zeros(4, 4), 2)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        be.denoise_svgf_torch(torch.zeros(4, 4, 3), m, 2)
    with pytest.raises(art.ArtError, match="dtype"):
        be.denoise_svgf_torch(torch.zeros(4, 4, 3, dtype=torch.float64), m, 2)
    with pytest.raises(art.ArtError, match="contiguous"):
        be.denoise_svgf_torch(torch.zeros(4, 3, 4).permute(0, 2, 1), m, 2)
    with pytest.raises(art.ArtError, match="variance_out: shape"):
        be.denoise_svgf_torch(torch.zeros(4, 4, 3), m, 2, variance_out=torch.zeros(4, 4, 1))
    with pytest.raises(TypeError, match="nope"):
        be.denoise_svgf_torch(torch.zeros(4, 4, 3), m, 2, nope=None)
