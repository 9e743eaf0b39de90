"""art_auto_exposure_device, art_display_device and art_exposure_state_bytes without a GPU: declared in the header, exported by the
library, listed in EXPORTED_SYMBOLS and bound in Ada; the structs match the header as compiled; the state's size is the header's layout;
what can be refused without a device is, each with its message; and the Python entries check their tensors before any C call."""
import ctypes as C
import os
import re
import subprocess

import pytest

NAMES = ("art_exposure_state_bytes", "art_auto_exposure_device", "art_display_device")
EXPOSURE_FIELDS = ("width", "height", "scale", "min_log2", "max_log2", "low_fraction", "high_fraction", "key", "adapt", "min_exposure", "max_exposure")
DISPLAY_FIELDS = ("width", "height", "scale", "exposure", "curve", "transfer", "white", "dither", "layout")
GOOD_E = (4, 4, 1.0, -12.0, 4.0, 0.5, 0.95, 0.18, 1.0, 1e-3, 1e3)
GOOD_D = (4, 4, 1.0, 1.0, 3, 1, 4.0, 1, 1)


def test_symbols_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int64_t\s+art_exposure_state_bytes\(void\);", hdr)
    assert re.search(r"int\s+art_auto_exposure_device\(const ArtExposureParams\* p, const float\* color3f, void\* state, void\* hip_stream\);", hdr)
    assert re.search(r"int\s+art_display_device\(const ArtDisplayParams\* p, const float\* color3f, const void\* exposure_state, uint32_t\* screen1u, float\* ldr3f,\s*"
                     r"void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    ads = open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    for name in NAMES:
        assert name in art.EXPORTED_SYMBOLS and getattr(art.load_library(), name) is not None
        assert re.search(r"\bT %s$" % name, out, flags=re.M)
        assert 'pragma Import (C, %s, "%s");' % (name, name) in ads
    for const in ("ART_CURVE_REFERENCE", "ART_CURVE_LINEAR", "ART_CURVE_REINHARD", "ART_CURVE_ACES", "ART_TRANSFER_SQRT", "ART_TRANSFER_SRGB", "ART_TRANSFER_GAMMA22"):
        assert re.search(r"\b%s = \d" % const, hdr) and re.search(r"\b%s : constant := \d;" % const, ads)
    assert (art.display.CURVE_REFERENCE, art.display.CURVE_LINEAR, art.display.CURVE_REINHARD, art.display.CURVE_ACES) == (0, 1, 2, 3)
    assert (art.display.TRANSFER_SQRT, art.display.TRANSFER_SRGB, art.display.TRANSFER_GAMMA22) == (0, 1, 2)


def test_structs_and_constants_match_the_header_as_compiled(art, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtExposureParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtExposureParams, %s));\n' % n for n in EXPOSURE_FIELDS)
                   + '  printf(" %zu", sizeof(ArtDisplayParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtDisplayParams, %s));\n' % n for n in DISPLAY_FIELDS)
                   + '  printf(" %d %d %d %d %d %d %d", ART_CURVE_REFERENCE, ART_CURVE_LINEAR, ART_CURVE_REINHARD, ART_CURVE_ACES, ART_TRANSFER_SQRT, ART_TRANSFER_SRGB, ART_TRANSFER_GAMMA22);\n'
                   + "  return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want_e, want_d = [44] + [4 * k for k in range(11)], [36] + [4 * k for k in range(9)]
    assert got == want_e + want_d + [0, 1, 2, 3, 0, 1, 2]
    ep, dp = art.display.ArtExposureParams, art.display.ArtDisplayParams
    assert [C.sizeof(ep)] + [getattr(ep, n).offset for n in EXPOSURE_FIELDS] == want_e
    assert [C.sizeof(dp)] + [getattr(dp, n).offset for n in DISPLAY_FIELDS] == want_d
    assert [t for _, t in ep._fields_] == [C.c_int32] * 2 + [C.c_float] * 9
    assert [t for _, t in dp._fields_] == [C.c_int32] * 2 + [C.c_float] * 2 + [C.c_int32] * 2 + [C.c_float] + [C.c_int32] * 2


def test_state_bytes_is_the_headers_layout(art):
    """four words (exposure, mean_log2, counted, frames) and 256 bins of 32 bits"""
    assert art.load_library().art_exposure_state_bytes() == 4 * (4 + 256) == 4 * art.display.STATE_WORDS == 1040
    hdr = open(os.path.join(art.ROOT, "include", "art_hip.h")).read()
    assert "art_exposure_state_bytes() = 1040 bytes" in hdr and "words 4 .. 259" in hdr


def test_exposure_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call)"""
    L = art.load_library()
    color, state = C.c_void_p(1 << 20), C.c_void_p(1 << 30)           # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")

    def refused(text, color=color, state=state, null_params=False, **kw):
        v = dict(zip(EXPOSURE_FIELDS, GOOD_E)); v.update(kw)
        par = art.display.ArtExposureParams(*[v[n] for n in EXPOSURE_FIELDS])
        rc = L.art_auto_exposure_device(None if null_params else C.byref(par), color, state, None)
        msg = L.art_last_error().decode()
        assert rc != 0 and msg.startswith("art_auto_exposure_device: ") and text in msg, (text, msg)
    refused("null ArtExposureParams", null_params=True)
    refused("null color3f or state", color=None)
    refused("null color3f or state", state=None)
    refused("width and height must be at least 1", width=0)
    refused("width and height must be at least 1", height=-3)
    refused("at most 2^28", width=1 << 15, height=1 << 14)
    refused("scale is not finite", scale=inf)
    refused("min_log2 < max_log2", min_log2=4.0)
    refused("min_log2 < max_log2", min_log2=5.0)
    refused("min_log2 < max_log2", max_log2=nan)
    refused("min_log2 < max_log2", min_log2=-200.0)
    refused("min_log2 < max_log2", max_log2=128.0)
    refused("low_fraction < high_fraction", low_fraction=0.95)
    refused("low_fraction < high_fraction", low_fraction=0.96)
    refused("low_fraction < high_fraction", low_fraction=-0.01)
    refused("low_fraction < high_fraction", high_fraction=1.01)
    refused("low_fraction < high_fraction", high_fraction=nan)
    refused("key must be finite and positive", key=0.0)
    refused("key must be finite and positive", key=-0.18)
    refused("key must be finite and positive", key=inf)
    refused("exposure bounds", min_exposure=0.0)
    refused("exposure bounds", max_exposure=-1.0)
    refused("exposure bounds", min_exposure=2.0, max_exposure=1.0)
    refused("exposure bounds", max_exposure=inf)
    refused("adapt must be in (0, 1]", adapt=0.0)
    refused("adapt must be in (0, 1]", adapt=-0.5)
    refused("adapt must be in (0, 1]", adapt=1.0001)
    refused("adapt must be in (0, 1]", adapt=nan)
    refused("state is not 4-byte aligned", state=C.c_void_p(state.value + 2))
    refused("state overlaps color3f", state=C.c_void_p(color.value + 12 * 16 - 4))
    refused("state overlaps color3f", state=C.c_void_p(color.value - 1040 + 4))


def test_display_refusals_that_need_no_device(art):
    L = art.load_library()
    color, state, screen, ldr = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 30), C.c_void_p(1 << 31)
    nan, inf = float("nan"), float("inf")

    def refused(text, color=color, state=None, screen=screen, ldr=ldr, null_params=False, **kw):
        v = dict(zip(DISPLAY_FIELDS, GOOD_D)); v.update(kw)
        par = art.display.ArtDisplayParams(*[v[n] for n in DISPLAY_FIELDS])
        rc = L.art_display_device(None if null_params else C.byref(par), color, state, screen, ldr, None)
        msg = L.art_last_error().decode()
        assert rc != 0 and msg.startswith("art_display_device: ") and text in msg, (text, msg)
    refused("null ArtDisplayParams", null_params=True)
    refused("null color3f", color=None)
    refused("screen1u and ldr3f are both null", screen=None, ldr=None)
    refused("width and height must be at least 1", width=0)
    refused("width and height must be at least 1", height=-1)
    refused("at most 2^28", width=1 << 15, height=1 << 14)
    refused("scale is not finite", scale=nan)
    refused("unknown curve", curve=4)
    refused("unknown curve", curve=-1)
    refused("unknown transfer", transfer=3)
    refused("unknown transfer", transfer=-1)
    refused("unknown layout", layout=2)
    refused("dither must be 0 or 1", dither=2)
    refused("white must be finite and positive", white=0.0)
    refused("white must be finite and positive", white=-4.0)
    refused("white must be finite and positive", white=inf)
    refused("white must be finite and positive", white=nan)
    refused("exposure must be finite and not negative", exposure=-1.0)
    refused("exposure must be finite and not negative", exposure=inf)
    refused("exposure must be finite and not negative", exposure=nan)
    refused("ldr3f is not defined for ART_CURVE_REFERENCE", curve=0)
    n = 16
    refused("screen1u overlaps color3f", screen=C.c_void_p(color.value + 12 * n - 4))
    refused("ldr3f overlaps color3f", ldr=C.c_void_p(color.value - 12 * n + 4))
    refused("ldr3f overlaps screen1u", ldr=C.c_void_p(screen.value + 4 * n - 4))
    refused("screen1u overlaps exposure_state", state=state, screen=C.c_void_p(state.value + 1040 - 4))
    refused("ldr3f overlaps exposure_state", state=state, ldr=C.c_void_p(state.value - 12 * n + 4))
    # with a state p->exposure is not read: the same bad value passes that check (and the call stops at the next one: no device here, or
    # the state is no device memory)
    par = art.display.ArtDisplayParams(*[dict(zip(DISPLAY_FIELDS, GOOD_D), exposure=nan)[k] for k in DISPLAY_FIELDS])
    assert L.art_display_device(C.byref(par), color, state, screen, ldr, None) != 0 and "exposure must be" not in L.art_last_error().decode()


def test_python_refuses_bad_tensors_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    color, state = torch.zeros(4, 5, 3), torch.zeros(art.display.STATE_WORDS, dtype=torch.int32)
    f, g = be.auto_exposure_torch, be.display_torch
    with pytest.raises(art.ArtError, match="color: a torch tensor"):
        f(None, state)
    with pytest.raises(art.ArtError, match=r"color: shape must be \[H, W, 3\]"):
        f(torch.zeros(4, 5), state)
    with pytest.raises(art.ArtError, match="color: dtype"):
        f(color.double(), state)
    with pytest.raises(art.ArtError, match="state: a torch tensor"):
        f(color, None)
    with pytest.raises(art.ArtError, match="state: dtype"):
        f(color, state.float())
    with pytest.raises(art.ArtError, match="state: shape"):
        f(color, state[:-1])
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(color, state)
    with pytest.raises(art.ArtError, match="color: a torch tensor"):
        g(None)
    with pytest.raises(art.ArtError, match="color: dtype"):
        g(color.half())
    with pytest.raises(art.ArtError, match="contiguous"):
        g(torch.zeros(5, 4, 3).transpose(0, 1))
    with pytest.raises(art.ArtError, match="state: shape"):
        g(color, state=state[:7])
    with pytest.raises(art.ArtError, match="out: dtype"):
        g(color, out=torch.zeros(4, 5))
    with pytest.raises(art.ArtError, match="out: shape"):
        g(color, out=torch.zeros(5, 4, dtype=torch.int32))
    with pytest.raises(art.ArtError, match="out: shape"):
        g(color, out=torch.zeros(4, 5, dtype=torch.int32), layout=art.LAYOUT_ADA_XY)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        g(color)
