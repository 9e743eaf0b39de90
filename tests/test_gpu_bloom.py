"""art_bloom_device on the GPU against the numpy reference written from the header (tests/bloom_ref.py): bit equality of out3f and
bloom3f on the shapes and settings the host test shares, planted bad values included; variant 0 (the small levels in one workgroup)
against variant 1 (one launch per level); in place against out of place and each output alone; a side stream; the properties the
header names; every refusal of tests/golden/bloom_refusals.json; and the chain pass -> bloom -> auto-exposure -> display end to end."""
import ctypes as C

import numpy as np
import pytest

import bloom_ref as R
import bloom_refusals as RF
import display_ref as D
import test_bloom_reference_host as TH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
U32 = np.uint32


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def state_tensor(exposure):
    s = D.new_state()
    s[0:1].view(F)[0] = exposure
    return dev(s.view(np.int32))


def gpu_bloom(backend, color, in_place=False, state_exposure=None, **kw):
    """bloom_ref.bloom's signature through Backend.bloom_torch: (out, bloom) as numpy; the reference's defaults, not the package's"""
    kw = dict(dict(levels=6, karis=1, scale=1.0, exposure=1.0, threshold=0.0, knee=0.0, scatter=0.7, strength=0.05, variant=0), **kw)
    c = dev(np.asarray(color, F))
    H, W = c.shape[:2]
    out = c if in_place else torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
    B = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
    st = None if state_exposure is None else state_tensor(state_exposure)
    got = backend.bloom_torch(c, st, out=out, bloom_out=B, **kw)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is B
    if not in_place:                                                  # (the input plane is only read)
        assert R.differ(c.cpu().numpy(), np.asarray(color, F)) == 0
    return out.cpu().numpy(), B.cpu().numpy()


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_kernels_equal_the_reference(backend, size):
    W, H = size
    for k, (name, kw) in enumerate(R.cases(W, H)):
        ref = R.bloom(**kw)[:2]
        assert R.differ_all(gpu_bloom(backend, **kw), ref) == 0, name
        assert R.differ_all(gpu_bloom(backend, **dict(kw, variant=1 - kw.get("variant", 0))), ref) == 0, name + " (the other variant)"
        if k % 4 == 0:
            assert R.differ_all(gpu_bloom(backend, in_place=True, **kw), ref) == 0, name + " (in place)"


def test_variant_0_equals_variant_1(backend):
    """641 x 363: the levels are 321 x 182, 161 x 91, 81 x 46, 41 x 23 (the tail's first: 943 + 252 + 66 + 18 + 6 records), so three
    levels have tiles of their own on either side of the tail, each with a partial last column and row of tiles"""
    W, H = 641, 363
    assert R.tail_first(W, H, 8) == 4 and R.launches(W, H, 8, 0) == 9 and R.launches(W, H, 8, 1) == 16
    c = R.planted_bad(R.frame(W, H, seed=2))
    for kw in (dict(levels=8, karis=1, scale=0.25, scatter=0.7, strength=0.25), dict(levels=6, karis=0, scale=0.25, threshold=1.0, knee=0.5, exposure=0.5, strength=1.0)):
        a, b = gpu_bloom(backend, c, variant=0, **kw), gpu_bloom(backend, c, variant=1, **kw)
        assert R.differ_all(a, b) == 0 and R.differ_all(a, R.bloom(c, **kw)[:2]) == 0 and a[1].any()


def test_in_place_and_each_output_alone(backend):
    """83 x 41 is 6 x 3 tiles of the frame, the last column and row partial: in place, every tile of the mix overwrites colour that the
    first downsample of a neighbouring tile has read -- in an earlier launch"""
    W, H = 83, 41
    c = R.planted_bad(R.frame(W, H, seed=3))
    kw = dict(levels=8, karis=1, scale=0.25, threshold=0.5, knee=0.5, exposure=0.5, scatter=0.6, strength=0.5)
    ref = R.bloom(c, **kw)[:2]
    assert R.differ_all(gpu_bloom(backend, c, **kw), ref) == 0 and R.differ_all(gpu_bloom(backend, c, in_place=True, **kw), ref) == 0
    cd = dev(c)
    out, none = backend.bloom_torch(cd, want_bloom=False, **kw)
    nothing, B = backend.bloom_torch(cd, want_out=False, **kw)
    torch.cuda.synchronize()
    assert none is None and nothing is None and R.differ(out.cpu().numpy(), ref[0]) == 0 and R.differ(B.cpu().numpy(), ref[1]) == 0


def test_side_stream_gives_the_context_streams_bits(backend):
    """the input copied on a torch side stream and the call enqueued there with no synchronisation in between, writing over its input;
    the exposure read from a state on the device"""
    W, H = 130, 70
    c = R.frame(W, H, seed=4)
    kw = dict(levels=8, karis=1, scale=0.25, threshold=1.0, knee=0.5, scatter=0.7, strength=0.3)
    ref = R.bloom(c, state_exposure=0.375, **kw)[:2]
    ch = torch.from_numpy(c).pin_memory()
    cd, B = torch.zeros((H, W, 3), device="cuda"), torch.zeros((H, W, 3), device="cuda")
    st = state_tensor(0.375)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cd.copy_(ch, non_blocking=True)
        got = backend.bloom_torch(cd, st, out=cd, bloom_out=B, **kw)
    side.synchronize()
    assert got[0] is cd and R.differ_all((cd.cpu().numpy(), B.cpu().numpy()), ref) == 0


@pytest.mark.parametrize("prop", TH.PROPERTIES, ids=lambda f: f.__name__)
def test_properties(backend, prop):
    prop(lambda c, **kw: gpu_bloom(backend, c, **kw))


def test_the_package_defaults(art, backend):
    """bloom_torch with nothing but the frame is the reference at the documented defaults"""
    c = R.frame(130, 70, seed=5)
    out, B = backend.bloom_torch(dev(c))
    torch.cuda.synchronize()
    b = art.bloom
    ref = R.bloom(c, levels=b.BLOOM_LEVELS, karis=b.BLOOM_KARIS, scatter=b.BLOOM_SCATTER, strength=b.BLOOM_STRENGTH, threshold=b.BLOOM_THRESHOLD, knee=b.BLOOM_KNEE)
    assert R.differ_all((out.cpu().numpy(), B.cpu().numpy()), ref[:2]) == 0


def test_every_refusal_of_the_fixture(art, backend):
    """every case of tests/golden/bloom_refusals.json over device planes: refused with its message and every plane still holds its
    sentinel; then the good call and the in-place call are accepted"""
    frame, cases = RF.load()
    sizes = RF.plane_bytes(frame)
    # every plane in a slot of two frames' bytes: a plane put 16 bytes into another one's slot reaches no third plane, so the refusal
    # names the overlap the case means
    slot = (2 * sizes["color3f"] + 255) // 256 * 256
    offsets = {k: i * slot for i, k in enumerate(RF.PLANES)}
    arena = torch.full((len(RF.PLANES) * slot,), 0x5a, dtype=torch.uint8, device="cuda")
    base = {k: arena.data_ptr() + offsets[k] for k in RF.PLANES}
    host = np.zeros(sizes["color3f"] // 4, F)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    held = []

    def short(nbytes):
        p = C.c_void_p(None)
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        held.append(p)
        return p.value

    def untouched():
        torch.cuda.synchronize()
        return bool((arena == 0x5a).all())
    try:
        for case in cases:
            RF.check(art, backend.lib, frame, case, base, host=host.ctypes.data, short=short)
            assert untouched(), case["name"]
    finally:
        torch.cuda.synchronize()
        for p in held:
            hip.hipFree(p)
    W, H = frame
    sentinel = np.full((H, W, 3), np.frombuffer(b"\x5a" * 4, F)[0], F)          # the arena's bytes as a frame: a constant 1.5e16
    for case in (dict(name="good"), dict(name="in place", args={"out3f": "is color3f"}), dict(name="no state", args={"exposure_state": "null"})):
        arena.fill_(0x5a)
        rc, text = RF.call(art, backend.lib, frame, case, base)
        torch.cuda.synchronize()
        assert rc == 0, (case["name"], text)
        got = arena[offsets["bloom3f"]:offsets["bloom3f"] + sizes["bloom3f"]].cpu().numpy().view(F).reshape(H, W, 3)
        kw = dict(levels=6, karis=1, threshold=1.0, knee=0.5, scatter=0.7, strength=0.05)
        e = dict(exposure=1.0) if case["name"] == "no state" else dict(state_exposure=float(sentinel[0, 0, 0]))
        assert R.differ(got, R.bloom(sentinel, **kw, **e)[1]) == 0, case["name"]
    # and from Python: the library's refusals as ArtError
    c = torch.zeros((H, W, 3), device="cuda")
    with pytest.raises(art.ArtError, match="art_bloom_device: levels must be 1 .. 8"):
        backend.bloom_torch(c, levels=9)
    with pytest.raises(art.ArtError, match="art_bloom_device: bloom3f overlaps color3f"):
        backend.bloom_torch(c, bloom_out=c)
    with pytest.raises(art.ArtError, match="art_bloom_device: out3f overlaps color3f"):
        big = torch.zeros(((H + 1) * W * 3,), device="cuda")                  # out3f one pixel into color3f
        backend.bloom_torch(big[:H * W * 3].view(H, W, 3), out=big[3:3 + H * W * 3].view(H, W, 3))
    if torch.cuda.device_count() > 1:                                         # another device's memory, where there is one
        with pytest.raises(art.ArtError):
            backend.bloom_torch(c, bloom_out=torch.zeros((H, W, 3), device="cuda:1"))


def test_end_to_end_pass_bloom_exposure_display(art, backend):
    """the 48 x 48 test scene: one 4-spp pass into a bound accum, bloom_torch on the bound tensor as it is (scale = 1 / 4),
    auto_exposure_torch and display_torch (ACES, sRGB, dither) on its result -- everything on the GPU -- equals bloom_ref -> display_ref
    fed the same accum words, on every HDR word, state word and screen word.  Then a second bloom with a threshold, which reads the
    exposure of that state on the device."""
    import temporal_quality as Q
    accum = torch.zeros((Q.H, Q.W, 3), dtype=torch.float32, device="cuda")
    try:
        backend.upload_scene(Q.scene(0))
        backend.bind_accum(accum)
        backend.set_camera(*Q.camera(0))
        backend.resize(Q.W, Q.H)
        spp = backend.render_pass_device(art.Backend.pass_params(art.PT_MIS, True, Q.DEPTH, 1, seed=Q.SEED), 0)
        assert spp == 4
        st = backend.exposure_state()
        out, B = backend.bloom_torch(accum, scale=1.0 / spp)
        backend.auto_exposure_torch(out, st)
        screen = backend.display_torch(out, st, curve=art.display.CURVE_ACES, transfer=art.display.TRANSFER_SRGB, dither=True)
        out2, B2 = backend.bloom_torch(accum, st, scale=1.0 / spp, threshold=1.0, knee=0.5, strength=0.5)
        torch.cuda.synchronize()
        words = accum.cpu().numpy()
        b = art.bloom
        r_out, r_B = R.bloom(words, levels=b.BLOOM_LEVELS, karis=b.BLOOM_KARIS, scale=0.25, scatter=b.BLOOM_SCATTER, strength=b.BLOOM_STRENGTH)[:2]
        assert R.differ(out.cpu().numpy(), r_out) == 0 and R.differ(B.cpu().numpy(), r_B) == 0 and r_B.any() and R.differ(r_out, R.sanitise(words, 0.25)) > 0
        r_state = D.auto_exposure(r_out, D.new_state())
        assert D.differ(st.cpu().numpy().view(U32), r_state) == 0 and r_state[2] > 0 and r_state[3] == 1
        r_screen = D.display(r_out, state=r_state, curve=D.CURVE_ACES, transfer=D.TRANSFER_SRGB, dither=1)[0]
        assert D.differ(screen.cpu().numpy().view(U32), r_screen) == 0 and len(np.unique(r_screen)) > 16
        r2 = R.bloom(words, levels=b.BLOOM_LEVELS, karis=b.BLOOM_KARIS, scale=0.25, scatter=b.BLOOM_SCATTER, strength=0.5, threshold=1.0, knee=0.5,
                     state_exposure=float(D.exposure_of(r_state)))[:2]
        assert R.differ_all((out2.cpu().numpy(), B2.cpu().numpy()), r2) == 0 and R.differ(r2[1], r_B) > 0
    finally:
        torch.cuda.synchronize()
        backend.bind_accum(None)
