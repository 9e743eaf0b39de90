"""The adaptive-sampling calls without a GPU: art_compact_mask_device, art_render_pass_masked and art_adaptive_estimate_device are declared
in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in Ada; ArtAdaptiveParams matches the header as compiled;
what can be refused without a device is; the Python layer refuses bad tensors before any C call."""
import ctypes as C
import os
import re
import subprocess

import pytest

NAMES = ("art_compact_mask_device", "art_render_pass_masked", "art_adaptive_estimate_device")
FIELDS = ("width", "height", "aa_on", "min_colours", "max_samples", "threshold", "lum_floor")


def test_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_compact_mask_device\(const uint8_t\* mask1b, uint32_t\* pixels_out, int64_t cap, uint32_t\* count_out, void\* hip_stream\);", hdr)
    assert re.search(r"int\s+art_render_pass_masked\(const ArtPassParams\* p, const uint8_t\* mask1b, uint32_t\* counts1u, int32_t\* spp_inout, int64_t\* pixels_out\);", hdr)
    assert re.search(r"int\s+art_adaptive_estimate_device\(const ArtAdaptiveParams\* p, const float\* accum3f, const float\* moments2f, const uint32_t\* counts1u,\s*"
                     r"float\* mean3f, float\* variance1f, float\* error1f, uint8_t\* mask1b, void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    for name in NAMES:
        assert name in art.EXPORTED_SYMBOLS and getattr(art.load_library(), name) is not None
        assert re.search(r"\bT %s$" % name, out, flags=re.M)
        assert 'pragma Import (C, %s, "%s");' % (name, name) in ads
    for method in ("compact_mask_torch", "render_pass_masked", "adaptive_estimate_torch", "render_adaptive"):
        assert hasattr(art.Backend, method)


def test_struct_matches_the_header_as_compiled(art, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtAdaptiveParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtAdaptiveParams, %s));\n' % n for n in FIELDS) + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [28, 0, 4, 8, 12, 16, 20, 24]
    assert got == want
    assert [C.sizeof(art.ArtAdaptiveParams)] + [getattr(art.ArtAdaptiveParams, n).offset for n in FIELDS] == want


def test_the_defaults_are_the_sweeps(art):
    import json
    best = json.load(open(os.path.join(art.ROOT, "profiles", "adaptive", "quality.json")))["best"]
    assert (art.ADAPTIVE_THRESHOLD, art.ADAPTIVE_LUM_FLOOR, art.ADAPTIVE_MIN_COLOURS) == (best["threshold"], best["lum_floor"], best["min_colours"])


def test_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call)"""
    L = art.load_library()
    one = C.c_void_p(16)                    # never dereferenced: every call below is refused on its parameters

    def refused(p, text, accum=one, mom=one, counts=one, mean=one):
        rc = L.art_adaptive_estimate_device(C.byref(p) if p is not None else None, accum, mom, counts, mean, None, None, None, None)
        assert rc != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())

    def params(**kw):
        p = art.ArtAdaptiveParams(4, 4, 1, 2, 64, 0.05, 0.01)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    refused(None, "art_adaptive_estimate_device: null ArtAdaptiveParams")
    refused(params(), "null accum3f, moments2f or counts1u", accum=None)
    refused(params(), "null accum3f, moments2f or counts1u", mom=None)
    refused(params(), "null accum3f, moments2f or counts1u", counts=None)
    refused(params(), "no output is wanted", mean=None)
    refused(params(width=0), "width and height")
    refused(params(width=1 << 15, height=1 << 14), "2^28")
    refused(params(min_colours=1), "min_colours")
    refused(params(max_samples=-1), "max_samples")
    refused(params(threshold=float("nan")), "threshold is NaN")
    refused(params(lum_floor=-1.0), "lum_floor")
    refused(params(lum_floor=float("inf")), "lum_floor")
    refused(params(lum_floor=float("nan")), "lum_floor")
    # the other two calls: no viewport, no scene
    assert L.art_compact_mask_device(None, one, 4, one, None) != 0 and "null mask1b" in L.art_last_error().decode()
    assert L.art_compact_mask_device(one, one, 4, one, None) != 0 and "no viewport" in L.art_last_error().decode()
    p = art.Backend.pass_params()
    assert L.art_render_pass_masked(C.byref(p), one, None, None, None) != 0 and "no scene" in L.art_last_error().decode()
    assert L.art_render_pass_masked(None, one, None, None, None) != 0 and "null ArtPassParams" in L.art_last_error().decode()


def test_python_refuses_bad_tensors_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    be.width, be.height = 4, 4
    p = art.Backend.pass_params()
    with pytest.raises(art.ArtError, match="mask: a torch tensor"):
        be.compact_mask_torch([1, 0])
    with pytest.raises(art.ArtError, match="mask: must be a GPU tensor"):
        be.compact_mask_torch(torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(art.ArtError, match="mask: must be a GPU tensor"):
        be.render_pass_masked(p, 0, torch.zeros(4, 4, dtype=torch.bool))
    with pytest.raises(art.ArtError, match="accum: a torch tensor"):
        be.adaptive_estimate_torch(None, None, None, True)
    with pytest.raises(art.ArtError, match="accum: must be a GPU tensor"):
        be.adaptive_estimate_torch(torch.zeros(48), torch.zeros(32), torch.zeros(16, dtype=torch.int32), True)
