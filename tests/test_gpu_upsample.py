"""art_upsample_device on the GPU against the numpy reference written from the header (tests/upsample_ref.py): bit equality of every out3f
word and every fallback1b byte on the shapes and cases the host test shares; the properties of tests/test_upsample_reference_host.py
asserted of the kernels; fallback1b through compact_mask_torch; a side stream; the refusals that need the device; and one end-to-end
frame: a 24 x 24 pass into a bound accum and the feature buffers at 24 x 24 and 48 x 48, upsampled on the GPU and by the reference from
the same downloaded planes."""
import ctypes as C

import numpy as np
import pytest

import test_upsample_reference_host as P
import upsample_ref as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_runner(backend):
    """upsample_ref.upsample's signature through Backend.upsample_torch: (out, fallback) as numpy arrays"""
    def run(lo_color, lo=None, hi=None, size=None, **kw):
        lo = {k: dev(v) for k, v in (lo or {}).items()}
        hi = {k: dev(v) for k, v in (hi or {}).items()}
        out = torch.full((size[1], size[0], 3), -7.0, device="cuda") if size is not None else None
        c = dev(np.asarray(lo_color, F))
        res, fb = backend.upsample_torch(c, lo, hi, want_fallback=True, out=out, **kw)
        torch.cuda.synchronize()
        assert out is None or res is out
        assert U.differ(c.cpu().numpy(), np.asarray(lo_color, F)) == 0      # (the input plane is only read)
        return res.cpu().numpy(), fb.cpu().numpy()
    return run


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_kernels_equal_the_reference(backend, shape):
    run = gpu_runner(backend)
    for name, kw, (out, fb) in U.reference_results(shape):
        gout, gfb = run(**kw)
        assert U.differ(out, gout) == 0, name + ": out3f"
        assert U.differ(fb, gfb) == 0, name + ": fallback1b"


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_no_guides_is_bilinear(backend, shape):
    P.no_guides_is_bilinear(gpu_runner(backend), shape)


@pytest.mark.parametrize("shape", P.PROPERTY_SHAPES, ids=U.SHAPE_IDS)
def test_id_boundary_keeps_the_sides_apart(backend, shape):
    P.id_boundary_keeps_the_sides_apart(gpu_runner(backend), shape)
    P.id_boundary_keeps_the_sides_apart(gpu_runner(backend), shape, U.GUIDES)


@pytest.mark.parametrize("shape", P.PROPERTY_SHAPES[1:], ids=U.SHAPE_IDS)
def test_background_is_not_flagged(backend, shape):
    P.background_is_not_flagged(gpu_runner(backend), shape)


def test_fallback_bytes_select_the_pixels_of_a_masked_pass(backend):
    """fallback1b handed to compact_mask_torch as it is: the count and the set of pixels are the reference's non-zero bytes"""
    W, H, LW, LH, jitter = shape = U.SHAPES[4]
    name, kw, (_, fb) = [r for r in U.reference_results(shape) if r[0] == "fp2_all_demod"][0]
    assert (fb == 1).any() and (fb == 2).any()
    c = dev(kw["lo_color"])
    _, gfb = backend.upsample_torch(c, {k: dev(v) for k, v in kw["lo"].items()}, {k: dev(v) for k, v in kw["hi"].items()}, footprint=2, jitter=jitter,
                                    scale=kw["scale"], demodulate=True, normal_log2=7, sigma_depth=1.0, want_fallback=True)
    backend.resize(W, H)
    pixels, count = backend.compact_mask_torch(gfb)
    torch.cuda.synchronize()
    n = int(count.item())
    assert n == int((fb != 0).sum())
    assert sorted(pixels[:n].cpu().numpy().view(np.uint32).tolist()) == np.flatnonzero(fb.reshape(-1)).tolist()


def test_side_stream_and_out_in_place(backend):
    """the planes copied on a torch side stream and the call enqueued there with no synchronisation in between; `out` is written in place"""
    shape = U.SHAPES[3]
    name, kw, (want, fb) = [r for r in U.reference_results(shape) if r[0] == "fp4_all_defaults"][0]
    host = dict(lo_color=torch.from_numpy(np.ascontiguousarray(kw["lo_color"])).pin_memory())
    lo_h = {k: torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for k, v in kw["lo"].items()}
    hi_h = {k: torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for k, v in kw["hi"].items()}
    c = torch.zeros_like(host["lo_color"], device="cuda")
    lo = {k: torch.zeros_like(v, device="cuda") for k, v in lo_h.items()}
    hi = {k: torch.zeros_like(v, device="cuda") for k, v in hi_h.items()}
    out = torch.full(want.shape, -7.0, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c.copy_(host["lo_color"], non_blocking=True)
        for k in lo:
            lo[k].copy_(lo_h[k], non_blocking=True)
            hi[k].copy_(hi_h[k], non_blocking=True)
        res, gfb = backend.upsample_torch(c, lo, hi, footprint=4, jitter=kw["jitter"], scale=kw["scale"], sigma_depth=0.5, out=out, want_fallback=True)
    side.synchronize()
    assert res is out and U.differ(out.cpu().numpy(), want) == 0 and U.differ(gfb.cpu().numpy(), fb) == 0


def test_refusals_that_need_the_device(art, backend):
    """host memory, a plane one pixel short and every overlap of an output with an input or the other output are refused, each by name, and
    nothing is written; bad tensors are refused from Python before that"""
    W, H, LW, LH = 41, 25, 20, 12
    lo_color, lo, hi = U.clean_planes(W, H, LW, LH)
    c, glo, ghi = dev(lo_color), {k: dev(v) for k, v in lo.items()}, {k: dev(v) for k, v in hi.items()}
    out = torch.full((H, W, 3), -7.0, device="cuda")
    fb = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
    L, Up = backend.lib, art.upsample
    host = np.zeros(3 * W * H, F)

    def call(text, color=c.data_ptr(), out_p=out.data_ptr(), fb_p=fb.data_ptr(), lo_kw=None, hi_kw=None):
        par = Up.ArtUpsampleParams(W, H, LW, LH, 2, 1, 5, 1.0, 1.0, (C.c_float * 2)(0.0, 0.0))
        a = dict({k: v.data_ptr() for k, v in glo.items()}, **(lo_kw or {}))
        b = dict({k: v.data_ptr() for k, v in ghi.items()}, **(hi_kw or {}))
        gl, gh = Up.ArtUpsampleGuides(*[a[k] for k in Up.GUIDES]), Up.ArtUpsampleGuides(*[b[k] for k in Up.GUIDES])
        rc = L.art_upsample_device(C.byref(par), color, C.byref(gl), C.byref(gh), out_p, fb_p, None)
        msg = L.art_last_error().decode() if rc else ""
        torch.cuda.synchronize()
        if text is None:
            assert rc == 0, msg
            return
        assert rc != 0 and text in msg, (text, msg)
        assert bool((out == -7.0).all()) and bool((fb == 9).all()), text
    call("lo_color3f is not device memory", color=host.ctypes.data)
    call("hi depth is not device memory", hi_kw=dict(depth=host.ctypes.data))
    call("lo id is not device memory", lo_kw=dict(id=host.ctypes.data))
    call("out3f is not device memory", out_p=host.ctypes.data)
    call("fallback1b is not device memory", fb_p=host.ctypes.data)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p(None)                                            # an allocation of its own, one pixel (1024 = N - 1 pixels: whole 4 KiB pages) short of a hi float3 plane
    assert hip.hipMalloc(C.byref(short), 12 * (W * H - 1)) == 0
    try:
        call("hi normal3f is smaller than the query needs", hi_kw=dict(normal=short.value))
    finally:
        hip.hipFree(short)
    call("out3f overlaps an input plane", out_p=ghi["albedo"].data_ptr())
    call("fallback1b overlaps an input plane", fb_p=ghi["id"].data_ptr())
    call("fallback1b overlaps an input plane", fb_p=c.data_ptr())
    call("fallback1b overlaps out3f", fb_p=out.data_ptr())
    call(None)                                                          # the unbroken call is accepted and writes both outputs
    want, wfb = U.upsample(lo_color, lo, hi, footprint=2, demodulate=True, normal_log2=5, sigma_depth=1.0)
    assert U.differ(out.cpu().numpy(), want) == 0 and U.differ(fb.cpu().numpy(), wfb) == 0
    with pytest.raises(art.ArtError, match="contiguous"):
        backend.upsample_torch(c, glo, dict(ghi, depth=torch.zeros((W, H), device="cuda").t()))
    with pytest.raises(art.ArtError, match="dtype"):
        backend.upsample_torch(c, glo, dict(ghi, id=ghi["id"].float()))
    with pytest.raises(art.ArtError, match="GPU tensor"):
        backend.upsample_torch(c, glo, dict(ghi, albedo=ghi["albedo"].cpu()))
    with pytest.raises(art.ArtError, match="out3f overlaps an input plane"):
        backend.upsample_torch(c, glo, ghi, out=ghi["normal"])


def test_end_to_end_on_the_test_scene(art, backend):
    """tests/temporal_quality.py's scene: a 24 x 24 pass into a bound accum and render_aovs_torch at 24 x 24 give the lo inputs,
    render_aovs_torch at 48 x 48 the hi guides; the upsample of these on the GPU equals the numpy reference fed with the same planes read
    back, bit for bit, and the frame is a picture (many colours, most pixels reconstructed by the guides)"""
    import temporal_quality as Q
    LW = LH = 24
    accum = torch.zeros((LH, LW, 3), dtype=torch.float32, device="cuda")
    p = art.Backend.pass_params(art.PT_MIS, False, Q.DEPTH, 1, seed=Q.SEED)
    names = ("albedo", "normal", "depth", "prim_index")
    try:
        backend.upload_scene(Q.scene(0))
        backend.bind_accum(accum)
        backend.set_camera(*Q.camera(0))
        backend.resize(LW, LH)
        spp = backend.render_pass_device(p, 0)
        lo = backend.render_aovs_torch(p, want=names)
        backend.bind_accum(None)
        backend.resize(Q.W, Q.H)
        hi = backend.render_aovs_torch(p, want=names)
        lo, hi = dict(lo, id=lo["prim_index"]), dict(hi, id=hi["prim_index"])
        for fp in (2, 4):
            out, fb = backend.upsample_torch(accum, lo, hi, footprint=fp, scale=1.0 / spp, want_fallback=True)
            torch.cuda.synchronize()
            want, wfb = U.upsample(accum.cpu().numpy(), {k: lo[k].cpu().numpy() for k in U.GUIDES}, {k: hi[k].cpu().numpy() for k in U.GUIDES}, footprint=fp,
                                   scale=1.0 / spp, sigma_depth=art.upsample.UPSAMPLE_SIGMA_DEPTH, normal_log2=art.upsample.UPSAMPLE_NORMAL_LOG2)
            assert U.differ(out.cpu().numpy(), want) == 0 and U.differ(fb.cpu().numpy(), wfb) == 0, fp
            assert tuple(out.shape) == (Q.H, Q.W, 3) and len(np.unique(want.reshape(-1, 3), axis=0)) > 256 and (wfb == 0).mean() > 0.5
    finally:
        torch.cuda.synchronize()
        backend.bind_accum(None)


def test_guided_upsampling_beats_plain_interpolation(art, backend):
    """the assertion of tests/test_upsample_quality.py of the kernels, on the same inputs: guided < ((1 + r) / 2) * unguided with the
    setting and the ratio r the sweep recorded (profiles/upsample/quality.json)"""
    import test_upsample_quality as TQ
    TQ.guided_beats_unguided(gpu_runner(backend), art)
