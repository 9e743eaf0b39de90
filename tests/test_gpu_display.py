"""art_auto_exposure_device and art_display_device on the GPU against the numpy reference written from the header (tests/display_ref.py):
bit equality of every screen word, ldr word, histogram bin and state word on the cases the host test shares; a side stream with each
choice of outputs; ART_CURVE_REFERENCE against art_download's screen of a rendered frame; the chain render -> feature buffers ->
temporal -> spatial variance -> filter -> auto-exposure -> display over two frames, end to end; and the refusals.

    python tests/test_gpu_display.py --record

writes tests/golden/display_refusals.json, the return code and the art_last_error() text of every refusal, from the library as it
stands (it needs the GPU); the test replays the table and compares byte for byte."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import display_ref as D

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "display_refusals.json")
F = np.float32
U32 = np.uint32
SIZE_IDS = lambda s: "%dx%d" % s


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def words(t):
    """a 32-bit tensor as the uint32 words it holds"""
    return t.cpu().numpy().view(U32)


def state_tensor(state):
    return dev(np.asarray(state, U32).view(np.int32))


def gpu_display(backend, color, state=None, want_screen=True, want_ldr=True, **kw):
    """display_ref.display's signature through Backend.display_torch: (screen words or None, ldr or None)"""
    want_ldr = want_ldr and kw.get("curve", D.CURVE_ACES) != D.CURVE_REFERENCE
    kw = dict(dict(curve=D.CURVE_ACES, transfer=D.TRANSFER_SRGB, white=4.0, dither=1, layout=D.LAYOUT_ROW_MAJOR), **kw)
    c = dev(color)
    res = backend.display_torch(c, None if state is None else state_tensor(state), want_ldr=want_ldr, want_screen=want_screen, **kw)
    torch.cuda.synchronize()
    assert D.differ(c.cpu().numpy(), np.asarray(color, F)) == 0      # (the input plane is only read)
    screen, ldr = res if want_ldr else (res, None)
    return (None if screen is None else words(screen)), (None if ldr is None else ldr.cpu().numpy())


@pytest.mark.parametrize("size", D.SIZES, ids=SIZE_IDS)
def test_exposure_kernels_equal_the_reference(backend, size):
    W, H = size
    for name, frames, kw in D.exposure_cases(W, H):
        ref, st = D.new_state(), backend.exposure_state()
        for k, frame in enumerate(frames):
            ref = D.auto_exposure(frame, ref, **kw)
            assert backend.auto_exposure_torch(dev(frame), st, **kw) is st
            got = words(st)
            assert D.differ(ref[4:], got[4:]) == 0, "%s, frame %d: histogram" % (name, k)
            assert D.differ(ref[:4], got[:4]) == 0, "%s, frame %d: state words %s != %s" % (name, k, ref[:4], got[:4])


@pytest.mark.parametrize("size", D.SIZES, ids=SIZE_IDS)
def test_display_kernel_equals_the_reference(backend, size):
    W, H = size
    for name, kw in D.display_cases(W, H):
        screen, ldr = D.display(**kw)
        gs, gl = gpu_display(backend, **kw)
        assert D.differ(screen, gs) == 0, name + ": screen"
        assert (ldr is None) == (gl is None) and (ldr is None or D.differ(ldr, gl) == 0), name + ": ldr"


def test_without_trimming_the_exposure_is_the_mean_of_the_bin_centres(backend):
    """the derived bound of tests/test_display_reference_host.py asserted of the kernels' state words, on the same frames: without
    trimming and with adapt = 1, -log2(exposure / key) is the mean of the counted pixels' bin centres to rounding (1e-5, as there) and
    within half a bin width, (max_log2 - min_log2) / 508, of the exact mean log2 luminance of a frame inside the range"""
    for W, H in D.SIZES[1:]:
        c = D.hdr_frame(W, H, 11, 1e-3, 15.0)
        l2 = np.log2(D.lum(c.reshape(-1, 3)).astype(np.float64))
        assert l2.min() > -12.0 and l2.max() < 4.0
        st = backend.auto_exposure_torch(dev(c), backend.exposure_state(), low_fraction=0.0, high_fraction=1.0, adapt=1.0)
        s = words(st)
        hist = s[4:].astype(np.float64)
        assert hist[0] == 0 and s[2] == W * H and s[3] == 1
        centres = -12.0 + ((np.arange(256) - 1 + 0.5) / 254.0) * 16.0
        mean_centres = (hist[1:255] * centres[1:255]).sum() / hist[1:255].sum()
        got = -np.log2(float(D.exposure_of(s)) / float(F(0.18)))
        print("%dx%d: -log2(exposure / key) %.6f, mean of centres %.6f, exact mean log2 luminance %.6f, bound %.6f" % (W, H, got, mean_centres, l2.mean(), 16.0 / 508))
        assert abs(got - mean_centres) < 1e-5 and abs(float(s[1:2].view(F)[0]) - mean_centres) < 1e-6
        assert abs(got - l2.mean()) <= 16.0 / 508


def test_side_stream_and_each_choice_of_outputs(backend):
    """the frame copied on a torch side stream and both calls enqueued there with no synchronisation in between: the display reads the
    exposure the call before it left in the state; screen only, ldr only and both give the same words, and `out` is written in place"""
    W, H = 70, 21
    c = D.special_frame(W, H, 7)
    kw = dict(curve=D.CURVE_REINHARD, transfer=D.TRANSFER_SRGB, white=2.5, dither=1, layout=D.LAYOUT_ADA_XY)
    ref_state = D.auto_exposure(c, D.new_state(), adapt=0.5)
    screen, ldr = D.display(c, state=ref_state, **kw)
    ch = torch.from_numpy(c).pin_memory()
    cd, st = torch.zeros((H, W, 3), device="cuda"), backend.exposure_state()
    out = torch.full((W, H), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cd.copy_(ch, non_blocking=True)
        backend.auto_exposure_torch(cd, st, adapt=0.5)
        both = backend.display_torch(cd, st, want_ldr=True, **kw)
        only_screen = backend.display_torch(cd, st, out=out, **kw)
        only_ldr = backend.display_torch(cd, st, want_ldr=True, want_screen=False, **kw)
    side.synchronize()
    assert D.differ(words(st), ref_state) == 0
    assert only_screen is out and only_ldr[0] is None
    assert D.differ(words(both[0]), screen) == 0 and D.differ(words(out), screen) == 0
    assert D.differ(both[1].cpu().numpy(), ldr) == 0 and D.differ(only_ldr[1].cpu().numpy(), ldr) == 0


def test_reference_curve_is_the_download_of_a_rendered_frame(art, backend):
    """the 48 x 48 test scene at 4 spp rendered into a bound accum: display_torch(accum, curve = REFERENCE, scale = 1 / spp) gives the
    screen words of download(spp), in both layouts"""
    import temporal_quality as Q
    accum = torch.zeros((Q.H, Q.W, 3), dtype=torch.float32, device="cuda")
    try:
        backend.upload_scene(Q.scene(0))
        backend.bind_accum(accum)
        backend.set_camera(*Q.camera(0))
        backend.resize(Q.W, Q.H)
        spp = backend.render_pass_device(art.Backend.pass_params(art.PT_MIS, True, Q.DEPTH, 1, seed=Q.SEED), 0)
        assert spp == 4
        for layout in (art.LAYOUT_ROW_MAJOR, art.LAYOUT_ADA_XY):
            _, want = backend.download(spp, layout)
            got = backend.display_torch(accum, curve=art.display.CURVE_REFERENCE, scale=1.0 / spp, layout=layout)
            torch.cuda.synchronize()
            assert len(np.unique(want)) > 16 and D.differ(words(got), want) == 0, layout
    finally:
        torch.cuda.synchronize()
        backend.bind_accum(None)


def test_end_to_end_two_frames_of_the_pan(art, backend):
    """two frames of tests/temporal_quality.py's pan at 48 x 48: render with accum and moments bound -> feature buffers -> temporal ->
    spatial variance -> variance-plane filter -> auto-exposure (adapt 0.5, one state) -> display (ACES, sRGB, dither), everything on the
    GPU; the reference run on the filtered planes read back gives the same state and screen words, and the second frame's state is not
    what a fresh state would have given: it depends on the first frame's"""
    import temporal_quality as Q
    accum = torch.zeros((Q.H, Q.W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((Q.H, Q.W, 2), dtype=torch.float32, device="cuda")
    st, ref = backend.exposure_state(), D.new_state()
    hist, prev = None, None
    try:
        backend.upload_scene(Q.scene(0))
        backend.bind_accum(accum)
        backend.bind_moments(moments)
        for k in range(2):
            p = art.Backend.pass_params(art.PT_MIS, True, Q.DEPTH, 1, seed=Q.SEED + k)
            backend.set_camera(*Q.camera(k))
            backend.resize(Q.W, Q.H)
            spp = backend.render_pass_device(p, 0)
            aovs = backend.render_aovs_torch(p, want=("albedo", "normal", "depth", "prim_index"))
            out, var, _, hist = backend.temporal_torch(dict(aovs, color=accum, moments=moments), hist, Q.camera(k), prev, spp // 4, scale=1.0 / spp)
            var = backend.svgf_spatial_variance_torch(hist, var, Q.W, Q.H, out=var)
            img = backend.denoise_svgf_torch(out, variance=var, albedo=aovs["albedo"], normal=aovs["normal"], depth=aovs["depth"])
            backend.auto_exposure_torch(img, st, adapt=0.5)
            screen = backend.display_torch(img, st, curve=art.display.CURVE_ACES, transfer=art.display.TRANSFER_SRGB, dither=True)
            torch.cuda.synchronize()
            plane = img.cpu().numpy()
            fresh = D.auto_exposure(plane, D.new_state(), adapt=0.5)
            ref = D.auto_exposure(plane, ref, adapt=0.5)
            assert D.differ(words(st), ref) == 0, "frame %d: state" % k
            assert D.differ(words(screen), D.display(plane, state=ref, curve=D.CURVE_ACES, transfer=D.TRANSFER_SRGB, dither=1)[0]) == 0, "frame %d: screen" % k
            assert ref[2] > 0 and ref[3] == k + 1 and len(np.unique(words(screen))) > 16
            assert (k == 0) == (D.differ(ref[:1], fresh[:1]) == 0)
            assert len(art.save_bmp(None, words(screen))) == 54 + 3 * Q.W * Q.H
            prev = Q.camera(k)
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
W, H = 41, 25                                                         # N - 1 = 1024 pixels: a plane short by one pixel is whole 4 KiB pages
N = W * H
SENTINEL = 0x5a5a5a5a
EXPOSURE_FIELDS = ("width", "height", "scale", "min_log2", "max_log2", "low_fraction", "high_fraction", "key", "adapt", "min_exposure", "max_exposure")
DISPLAY_FIELDS = ("width", "height", "scale", "exposure", "curve", "transfer", "white", "dither", "layout")
GOOD_E = (W, H, 1.0, -12.0, 4.0, 0.5, 0.95, 0.18, 1.0, 1e-3, 1e3)
GOOD_D = (W, H, 1.0, 1.0, D.CURVE_ACES, D.TRANSFER_SRGB, 4.0, 1, D.LAYOUT_ROW_MAJOR)
NAN, INF = float("nan"), float("inf")
BAD_E = [("size", dict(width=0)), ("size", dict(height=-1)), ("size", dict(width=1 << 15, height=1 << 14)), ("scale", dict(scale=INF)),
         ("log2 range", dict(min_log2=4.0)), ("log2 range", dict(min_log2=6.0)), ("log2 range", dict(max_log2=NAN)), ("fractions", dict(low_fraction=0.95)),
         ("fractions", dict(low_fraction=-0.5)), ("fractions", dict(high_fraction=1.5)), ("fractions", dict(low_fraction=0.9, high_fraction=0.1)),
         ("key", dict(key=0.0)), ("key", dict(key=-1.0)), ("exposure bounds", dict(min_exposure=0.0)), ("exposure bounds", dict(max_exposure=-1.0)),
         ("adapt", dict(adapt=0.0)), ("adapt", dict(adapt=1.5)), ("adapt", dict(adapt=NAN))]
BAD_D = [("size", dict(width=0)), ("size", dict(width=1 << 15, height=1 << 14)), ("scale", dict(scale=NAN)), ("curve", dict(curve=4)), ("curve", dict(curve=-1)),
         ("transfer", dict(transfer=3)), ("layout", dict(layout=2)), ("dither", dict(dither=2)), ("white", dict(white=0.0)), ("white", dict(white=-1.0)),
         ("white", dict(white=NAN))]


def collect(art, backend):
    """{call/case: [rc, art_last_error() text]}: every bad parameter, every pointer on the host and one pixel short, no output, an output
    over the input or the state.  After every refused call the outputs still hold the sentinel (nothing was launched); after each group of
    refusals the unbroken calls are made, are accepted and write their outputs (accepted()), and the sentinels are put back."""
    L = backend.lib
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    color = dev(D.hdr_frame(W, H, 1))
    state = torch.full((art.display.STATE_WORDS,), SENTINEL, dtype=torch.int32, device="cuda")
    screen = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
    ldr = torch.full((3 * N,), SENTINEL, dtype=torch.int32, device="cuda")
    host = np.zeros(3 * N, F)
    got = {}

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in (state, screen, ldr))

    def untouched_state():
        return bool((state == SENTINEL).all())

    def exposure(case, expect_refusal=True, color=color.data_ptr(), state=state.data_ptr(), null_params=False, **kw):
        v = dict(zip(EXPOSURE_FIELDS, GOOD_E)); v.update(kw)
        p = art.display.ArtExposureParams(*[v[n] for n in EXPOSURE_FIELDS])
        rc = L.art_auto_exposure_device(None if null_params else C.byref(p), color, state, None)
        text = L.art_last_error().decode() if rc else ""
        ident = "art_auto_exposure_device/%s" % case
        assert ident not in got and (rc != 0) == expect_refusal and (not expect_refusal or (text != "" and untouched())), (ident, rc, text)
        got[ident] = [rc, text]

    def display(case, expect_refusal=True, color=color.data_ptr(), state=None, screen=screen.data_ptr(), ldr=ldr.data_ptr(), null_params=False, **kw):
        v = dict(zip(DISPLAY_FIELDS, GOOD_D)); v.update(kw)
        p = art.display.ArtDisplayParams(*[v[n] for n in DISPLAY_FIELDS])
        rc = L.art_display_device(None if null_params else C.byref(p), color, state, screen, ldr, None)
        text = L.art_last_error().decode() if rc else ""
        ident = "art_display_device/%s" % case
        assert ident not in got and (rc != 0) == expect_refusal and (not expect_refusal or (text != "" and untouched())), (ident, rc, text)
        got[ident] = [rc, text]

    def short(bytes_, call):
        p = C.c_void_p(None)
        assert hip.hipMalloc(C.byref(p), bytes_) == 0
        try:
            call(p.value)
        finally:
            hip.hipFree(p)

    def accepted(after):
        """the next valid calls after a group of refusals succeed and write: the state first (the display reads it), then both outputs"""
        exposure("accepted after %s" % after, expect_refusal=False)
        display("accepted after %s" % after, expect_refusal=False, state=state.data_ptr())
        torch.cuda.synchronize()
        assert int(words(state)[4:].sum()) == N and not bool((screen == SENTINEL).any()) and not bool((ldr == SENTINEL).any()), after
        for t in (state, screen, ldr):
            t.fill_(SENTINEL)
        assert untouched()

    exposure("null params", null_params=True)
    exposure("null color3f", color=None)
    exposure("null state", state=None)
    for k, (what, kw) in enumerate(BAD_E):
        exposure("%s %s" % (what, sorted(kw.items())), **kw)
    exposure("state over color3f", state=color.data_ptr() + 64)
    exposure("state misaligned", state=state.data_ptr() + 2)
    accepted("the exposure's parameters")
    exposure("color3f on the host", color=host.ctypes.data)
    exposure("state on the host", state=host.ctypes.data)
    short(12 * (N - 1), lambda p: exposure("color3f one pixel short", color=p))
    short(4096, lambda p: exposure("state too small", state=p + 4096 - 1036))
    accepted("the exposure's pointers")
    display("null params", null_params=True)
    display("null color3f", color=None)
    display("no output", screen=None, ldr=None)
    for what, kw in BAD_D:
        display("%s %s" % (what, sorted(kw.items())), **kw)
    for bad in (-1.0, INF, NAN):
        display("exposure %r without a state" % bad, exposure=bad)
    display("ldr3f with the reference curve", curve=D.CURVE_REFERENCE)
    accepted("the display's parameters")
    display("screen1u over color3f", screen=color.data_ptr() + 12 * N - 4)
    display("ldr3f over color3f", ldr=color.data_ptr())
    display("ldr3f over screen1u", ldr=screen.data_ptr())
    display("screen1u over exposure_state", state=state.data_ptr(), screen=state.data_ptr() + 1036)
    display("ldr3f over exposure_state", state=state.data_ptr(), ldr=state.data_ptr())
    accepted("the display's overlaps")
    display("color3f on the host", color=host.ctypes.data)
    display("exposure_state on the host", state=host.ctypes.data)
    display("screen1u on the host", screen=host.ctypes.data)
    display("ldr3f on the host", ldr=host.ctypes.data)
    short(12 * (N - 1), lambda p: display("color3f one pixel short", color=p))
    short(4096, lambda p: display("exposure_state too small", state=p + 4096 - 1036))
    short(4 * (N - 1), lambda p: display("screen1u one pixel short", screen=p))
    short(12 * (N - 1), lambda p: display("ldr3f one pixel short", ldr=p))
    accepted("the display's pointers")
    # and each choice of outputs
    display("accepted, screen only", expect_refusal=False, ldr=None)
    display("accepted, ldr only", expect_refusal=False, screen=None)
    display("accepted, the reference curve", expect_refusal=False, curve=D.CURVE_REFERENCE, ldr=None)
    torch.cuda.synchronize()
    assert not bool((screen == SENTINEL).any()) and not bool((ldr == SENTINEL).any()) and untouched_state()
    return got


def test_every_refusal_is_the_recorded_one(art, backend):
    got = collect(art, backend)
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    assert sorted(got) == sorted(want)
    wrong = ["%s: got %r, recorded %r" % (k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "\n".join(wrong)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path[:0] = [HERE, os.path.dirname(HERE)]
    import __graft_entry__ as ge
    pkg = ge.load_package()
    be = pkg.Backend(0)
    cases = collect(pkg, be)
    be.shutdown()
    with open(GOLDEN, "w") as f:
        json.dump({"frame": [W, H], "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(cases), GOLDEN))
