"""art_temporal_upsample_device without a GPU: declared in the header, exported by the library, listed in EXPORTED_SYMBOLS and bound in
Ada; the structs match the header as compiled; what can be refused without a device is, each with its message
(tests/golden/temporal_upsample_refusals.json); the Python entry checks its tensors before any C call; the jitter sequence and the
jittered camera are what their documentation says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_upsample_refusals as RF

NAME = RF.NAME
PARAM_FIELDS = ("t", "lo_width", "lo_height", "jitter", "radius", "min_confidence")
GUIDE_FIELDS = ("normal3f", "depth", "id", "motion3f")


def test_symbol_declared_and_exported(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+art_temporal_upsample_device\(const ArtTemporalUpsampleParams\* p, const float\* lo_color3f, const float\* lo_moments2f,\s*"
                     r"const ArtTemporalUpsampleGuides\* lo, const ArtTemporalUpsampleGuides\* hi,\s*const void\* hist_in\s*, void\* hist_out, float\* out3f, "
                     r"float\* variance_out, float\* length_out,\s*uint8_t\* fallback1b, void\* hip_stream\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", art.LIB_PATH], text=True)
    assert NAME in art.EXPORTED_SYMBOLS and getattr(art.load_library(), NAME) is not None
    assert re.search(r"\bT %s$" % NAME, out, flags=re.M)
    assert 'pragma Import (C, %s, "%s");' % (NAME, NAME) in open(os.path.join(art.PKG_DIR, "ada", "art_hip.ads")).read()
    assert hasattr(art.Backend, "temporal_upsample_torch")


def test_structs_match_the_header_as_compiled(art, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "art_hip.h"\nint main(void) { printf("%zu", sizeof(ArtTemporalUpsampleParams));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtTemporalUpsampleParams, %s));\n' % n for n in PARAM_FIELDS)
                   + '  printf(" %zu", sizeof(ArtTemporalUpsampleGuides));\n'
                   + "".join('  printf(" %%zu", offsetof(ArtTemporalUpsampleGuides, %s));\n' % n for n in GUIDE_FIELDS)
                   + '  printf(" %zu", sizeof(ArtTemporalParams));\n  return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(art.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want_p, want_g = [212, 0, 188, 192, 196, 204, 208], [32, 0, 8, 16, 24]
    assert got == want_p + want_g + [188]
    tp, tg = art.temporal_upsample.params_struct(), art.temporal_upsample.ArtTemporalUpsampleGuides
    assert [C.sizeof(tp)] + [getattr(tp, n).offset for n in PARAM_FIELDS] == want_p
    assert [C.sizeof(tg)] + [getattr(tg, n).offset for n in GUIDE_FIELDS] == want_g
    assert [t for _, t in tp._fields_] == [art.ArtTemporalParams, C.c_int32, C.c_int32, C.c_float * 2, C.c_float, C.c_float]
    assert [t for _, t in tg._fields_] == [C.c_void_p] * 4


def fake_planes(frame):
    """addresses that are never dereferenced, far enough apart that no two planes overlap"""
    return {k: (1 << 32) + (k_ << 28) for k_, k in enumerate(RF.PLANES)}


def test_refusals_that_need_no_device(art):
    """the parameter checks come before the device is looked for: each names its reason (no GPU is touched by a refused call)"""
    L = art.load_library()
    frame, cases = RF.load()
    ran = 0
    for case in cases:
        if not case["needs_device"]:
            RF.check(art, L, frame, case, fake_planes(frame))
            ran += 1
    assert ran >= 40
    # the good call passes every one of these and stops at the next check (no device here, or the pointers are no device memory)
    rc, text = RF.call(art, L, frame, dict(name="good", set=dict(jitter0=0.49, jitter1=-0.49, radius=float(np.float32(25) / np.float32(13)), min_confidence=1.0)),
                       fake_planes(frame))
    assert rc != 0 and not any(t in text for t in ("jitter", "one side", "must be", "null ", "refused", "overlap"))


def test_python_refuses_bad_tensors_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    f = be.temporal_upsample_torch
    cam = (np.zeros(3, np.float32), np.eye(4, dtype=np.float32))
    lc, lm = torch.zeros(3, 4, 3), torch.zeros(3, 4, 2)
    lo = dict(normal=torch.zeros(3, 4, 3), depth=torch.zeros(3, 4), id=torch.zeros(3, 4, dtype=torch.int32))
    hi = dict(normal=torch.zeros(6, 8, 3), depth=torch.zeros(6, 8), id=torch.zeros(6, 8, dtype=torch.int32))
    with pytest.raises(art.ArtError, match="color: a torch tensor"):
        f(None, lm, lo, hi, cam)
    with pytest.raises(art.ArtError, match=r"color: shape must be \[H, W, 3\]"):
        f(torch.zeros(3, 4), lm, lo, hi, cam)
    with pytest.raises(art.ArtError, match="lo_color: dtype"):
        f(lc.double(), lm, lo, hi, cam)
    with pytest.raises(art.ArtError, match="lo_moments: a torch tensor"):
        f(lc, None, lo, hi, cam)
    with pytest.raises(art.ArtError, match="lo_moments: shape must hold at least 24 elements"):
        f(lc, torch.zeros(3, 4), lo, hi, cam)
    with pytest.raises(art.ArtError, match="lo: a dict of planes is required"):
        f(lc, lm, None, hi, cam)
    with pytest.raises(art.ArtError, match="hi: a dict of planes is required"):
        f(lc, lm, lo, [1], cam)
    with pytest.raises(art.ArtError, match="motion is the hi frame's plane"):
        f(lc, lm, dict(lo, motion=torch.zeros(3, 4, 3)), hi, cam)
    with pytest.raises(art.ArtError, match="depth is given on one side only"):
        f(lc, lm, dict(lo, depth=None), hi, cam)
    with pytest.raises(art.ArtError, match="id is given on one side only"):
        f(lc, lm, lo, {k: v for k, v in hi.items() if k != "id"}, cam)
    with pytest.raises(art.ArtError, match=r"lo\['normal'\]: shape"):
        f(lc, lm, dict(lo, normal=torch.zeros(3, 5, 3)), hi, cam)
    with pytest.raises(art.ArtError, match=r"hi\['depth'\]: shape"):
        f(lc, lm, lo, dict(hi, depth=torch.zeros(6, 8, 1)), cam)
    with pytest.raises(art.ArtError, match=r"hi\['id'\]: dtype"):
        f(lc, lm, lo, dict(hi, id=torch.zeros(6, 8)), cam)
    with pytest.raises(art.ArtError, match=r"hi\['motion'\]: shape"):
        f(lc, lm, lo, dict(hi, motion=torch.zeros(6, 8)), cam)
    with pytest.raises(art.ArtError, match="hist_in: shape"):
        f(lc, lm, lo, hi, cam, cam, hist_in=torch.zeros(6, 8, 4))
    with pytest.raises(art.ArtError, match="contiguous"):
        f(lc, lm, lo, dict(hi, depth=torch.zeros(8, 6).t()), cam)
    with pytest.raises(art.ArtError, match="prev: a history needs the camera"):
        f(lc, lm, lo, hi, cam, None, hist_in=torch.zeros(3, 6, 8, 4))
    with pytest.raises(art.ArtError, match="cur: a camera is"):
        f(lc, lm, lo, hi, None)
    with pytest.raises(art.ArtError, match="cur: a camera is"):
        f(lc, lm, lo, hi, (1, 2, 3))
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(lc, lm, lo, hi, cam)
    with pytest.raises(art.ArtError, match="GPU tensor"):
        f(lc, lm, {}, {}, cam, size=(8, 6))


def test_jitter_sequence_is_halton_2_3_inside_the_open_interval(art):
    j = art.temporal_upsample.jitter_sequence(64)
    assert j.shape == (64, 2) and j.dtype == np.float32
    assert (np.abs(j) < 0.5).all()
    assert np.allclose(j[:4], [[0.0, 1 / 3 - 0.5], [-0.25, 2 / 3 - 0.5], [0.25, 1 / 9 - 0.5], [-0.375, 4 / 9 - 0.5]], atol=1e-7)
    # every 2 x 2 quarter of the pixel is visited within four frames in x, and the sequence spreads over the pixel
    assert len({(int(a >= 0), int(b >= 0)) for a, b in j[:8]}) == 4
    assert abs(float(j.mean())) < 0.02
    assert art.temporal_upsample.jitter_sequence(0).shape == (0, 2)


def test_jittered_camera_is_the_shear_that_moves_the_ray_grid(art):
    """M' r = M (r + (jx, jy, 0)) for every r with r.z = cam_z = -lo_width, in binary64 up to the rounding of M' to binary32"""
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = q.astype(np.float32)
    lw, jit = 24, (0.25, -0.375)
    ms = art.temporal_upsample.jittered_camera(m, lw, jit)
    assert ms.dtype == np.float32 and ms.shape == (4, 4) and (ms[:, 3] == m[:, 3]).all() and (ms[3] == m[3]).all()
    assert (ms[:3, :2] == m[:3, :2]).all()
    r = np.stack([rng.uniform(-12, 12, 50), rng.uniform(-12, 12, 50), np.full(50, -float(lw))], -1)
    want = (r + np.array([jit[0], jit[1], 0.0])) @ m[:3, :3].astype(np.float64).T
    got = r @ ms[:3, :3].astype(np.float64).T
    assert np.abs(got - want).max() < 24 * 2.0 ** -23
    assert (art.temporal_upsample.jittered_camera(m, lw, (0.0, 0.0)) == m).all()
