"""art_denoise_svgf_device on the GPU against the numpy reference written from the header (tests/svgf_ref.py): bit equality of the colour
and of variance_out on small frames, in place, with non-finite inputs, on a side stream, end to end behind a render with both tensors
bound, and every refusal.  art_denoise_device on the same inputs is still its own reference's (nothing existing moved)."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as R
import svgf_quality as Q
import svgf_ref as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(backend, color, mom, nc, g, kw, **more):
    H, W = color.shape[:2]
    var = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
    out = backend.denoise_svgf_torch(dev(color), dev(mom), nc, **{k: dev(v) for k, v in g.items()}, **kw, variance_out=var, **more)
    torch.cuda.synchronize()
    return out.cpu().numpy(), var.cpu().numpy()


_want = {}


def want(size, c):
    """the reference's (colour, variance) of one size and combination: computed once, read-only"""
    key = (size, c)
    if key not in _want:
        W, H = size
        color, mom, nc, g, kw = S.combo_args(R.planes(W, H), c, W, H)
        _want[key] = S.denoise(color, mom, nc, **g, **kw)
    return _want[key]


@pytest.mark.parametrize("size", S.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_reference(backend, size):
    W, H = size
    pl = R.planes(W, H)
    for c in S.combos():
        if c[0] > 3 and size != (37, 23):
            continue                                    # iterations 5 and 8: on 37x23 only (spacing 16 and 128 against the frame)
        color, mom, nc, g, kw = S.combo_args(pl, c, W, H)
        got, ref = run(backend, color, mom, nc, g, kw), want(size, c)
        assert S.differ(got[0], ref[0]) == 0 and S.differ(got[1], ref[1]) == 0, S.combo_id(c)


def test_plain_denoiser_is_what_it_was(backend):
    W, H = 37, 23
    pl = R.planes(W, H)
    for c in R.combos()[::17]:
        color, g, kw = R.combo_args(pl, c)
        out = backend.denoise_torch(dev(color), **{k: dev(v) for k, v in g.items()}, **kw).cpu().numpy()
        assert R.differ(out, R.denoise(color, **g, **kw)) == 0, R.combo_id(c)


def test_in_place_and_without_variance_out(backend):
    W, H = 37, 23
    color, albedo, normal, depth = R.planes(W, H)
    mom = S.moments_for(color, 4, W, H)
    ref = S.denoise(color, mom, 4, albedo, normal, depth, iterations=3, scale=0.5, sigma_color=4.0)
    same = dev(color)
    ret = backend.denoise_svgf_torch(same, dev(mom), 4, dev(albedo), dev(normal), dev(depth), iterations=3, scale=0.5, sigma_color=4.0, out=same)
    assert ret is same and S.differ(same.cpu().numpy(), ref[0]) == 0
    flat = dev(mom.reshape(-1))                                          # the tensor of bind_moments as it is: flat
    apart = backend.denoise_svgf_torch(dev(color), flat, 4, dev(albedo), dev(normal), dev(depth), iterations=3, scale=0.5, sigma_color=4.0, alpha=None, mat=None)
    assert S.differ(apart.cpu().numpy(), ref[0]) == 0


def test_non_finite_inputs(backend):
    W, H = 37, 23
    color, albedo, normal, depth = [x.copy() for x in R.planes(W, H)]
    mom = S.moments_for(color, 4, W, H)
    color[9, 20] = np.nan; color[20, 30, 1] = np.inf
    mom[9, 9, 1] = np.inf; mom[10, 3] = np.nan; mom[2, 30, 0] = -np.inf
    depth[12, 20] = np.nan; normal[15, 5, 0] = np.nan
    for it in (1, 3):
        kw = dict(iterations=it, scale=0.25, sigma_color=4.0)
        got, ref = run(backend, color, mom, 4, dict(albedo=albedo, normal=normal, depth=depth), kw), S.denoise(color, mom, 4, albedo, normal, depth, **kw)
        assert S.differ(got[0], ref[0]) == 0 and S.differ(got[1], ref[1]) == 0
        assert np.isfinite(got[0]).all() and (got[1] >= 0).all()          # repaired
    clean = R.planes(W, H)
    a = S.denoise(clean[0], S.moments_for(clean[0], 4, W, H), 4, albedo, clean[2], clean[3], iterations=1, scale=0.25, sigma_color=4.0)[0]
    b = run(backend, color, mom, 4, dict(albedo=albedo, normal=normal, depth=depth), dict(iterations=1, scale=0.25, sigma_color=4.0))[0]
    far = np.ones((H, W), bool)
    for (y, x) in ((9, 20), (20, 30), (9, 9), (10, 3), (2, 30), (12, 20), (15, 5)):
        far[max(0, y - 3):y + 4, max(0, x - 3):x + 4] = False
    assert np.array_equal(a.view(np.uint32)[far], b.view(np.uint32)[far])  # not spread


def test_stream_order_on_a_side_stream(backend):
    """the inputs are written on a torch side stream and the filter is enqueued there with no synchronisation in between"""
    W, H = 300, 5
    color, albedo, normal, depth = R.planes(W, H)
    mom = S.moments_for(color, 8, W, H)
    host = [torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in (color, mom, albedo, normal, depth)]
    d = [torch.zeros_like(x, device="cuda") for x in host]
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for a, b in zip(d, host):
            a.copy_(b, non_blocking=True)
        out = backend.denoise_svgf_torch(d[0], d[1], 8, d[2], d[3], d[4], iterations=3, scale=0.25, sigma_color=4.0, variance_out=var)
    st.synchronize()
    ref = S.denoise(color, mom, 8, albedo, normal, depth, iterations=3, scale=0.25, sigma_color=4.0)
    assert S.differ(out.cpu().numpy(), ref[0]) == 0 and S.differ(var.cpu().numpy(), ref[1]) == 0


def test_refusals(art, backend):
    W, H = 41, 25                                                    # N - 1 = 1024 pixels: the short planes below are whole 4 KiB pages
    L = backend.lib
    N = W * H
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    color, mom, out, var = [torch.zeros(k * N, dtype=torch.float32, device="cuda") for k in (3, 2, 3, 1)]
    guide3, guide1 = torch.ones(3 * N, dtype=torch.float32, device="cuda"), torch.ones(N, dtype=torch.float32, device="cuda")
    host = np.zeros(3 * N, F)
    good = [color.data_ptr(), mom.data_ptr(), guide3.data_ptr(), guide3.data_ptr(), guide1.data_ptr(), out.data_ptr(), var.data_ptr()]

    def params(**kw):
        d = dict(width=W, height=H, iterations=2, demodulate=1, normal_log2=7, n_colours=4, scale=1.0, sigma_color=2.0, sigma_depth=1.0)
        d.update(kw)
        return art.ArtSvgfParams(**d)

    def refused(p, ptrs, text):
        before = out.clone()
        rc = L.art_denoise_svgf_device(C.byref(p) if p is not None else None, *ptrs, None)
        torch.cuda.synchronize()
        assert rc != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())
        assert torch.equal(out, before)

    def but(i, v):
        p = list(good); p[i] = v
        return p
    refused(None, good, "null ArtSvgfParams")
    refused(params(), but(0, None), "null color3f or out3f")
    refused(params(), but(5, None), "null color3f or out3f")
    refused(params(), but(1, None), "null moments2f")
    for n in (1, 0, -3):
        refused(params(n_colours=n), good, "n_colours")
    for kw, text in ((dict(width=0), "width"), (dict(height=-1), "width"), (dict(width=1 << 15, height=1 << 14), "width"), (dict(iterations=0), "iterations"),
                     (dict(iterations=9), "iterations"), (dict(normal_log2=11), "normal_log2"), (dict(normal_log2=-1), "normal_log2"),
                     (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"), (dict(sigma_color=float("nan")), "sigma"),
                     (dict(sigma_depth=float("nan")), "sigma")):
        refused(params(**kw), good, text)
    for i, (name, per) in enumerate((("color3f", 12), ("moments2f", 8), ("albedo3f", 12), ("normal3f", 12), ("depth", 4), ("out3f", 12), ("variance_out", 4))):
        refused(params(), but(i, host.ctypes.data), name + " is not device memory")
        short = C.c_void_p(None)                                     # an allocation of its own, too small by one pixel
        assert hip.hipMalloc(C.byref(short), (N - 1) * per) == 0
        try:
            refused(params(), but(i, short.value), name + " is smaller than")
        finally:
            hip.hipFree(short)
    assert L.art_denoise_svgf_device(C.byref(params()), *good, None) == 0              # and the same arguments, unbroken, are accepted
    assert L.art_denoise_svgf_device(C.byref(params()), *but(6, None), None) == 0       # variance_out is optional
    assert L.art_denoise_svgf_device(C.byref(params()), *good[:2], None, None, None, *good[5:], None) == 0
    torch.cuda.synchronize()
    with pytest.raises(art.ArtError, match="n_colours"):
        backend.denoise_svgf_torch(color.view(H, W, 3), mom, 1)


def frame_planes(art, backend, sd, W, H, p, passes):
    """accum and moments bound, `passes` passes, the feature buffers: everything stays on the GPU"""
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    backend.upload_scene(sd)
    backend.bind_accum(accum)
    backend.bind_moments(moments)
    backend.resize(W, H)
    spp = 0
    for _ in range(passes):
        spp = backend.render_pass_device(p, spp)
    aovs = backend.render_aovs_torch(p, want=("albedo", "normal", "depth", "alpha"))
    return accum, moments, spp, aovs


def unbind(backend):
    torch.cuda.synchronize()
    backend.bind_moments(None)
    backend.bind_accum(None)


def test_end_to_end(art, backend):
    """bind both tensors, two PT_MIS passes with anti-aliasing (8 spp, 2 colours), the feature buffers, the filter with its defaults: the
    output and the variance are the reference's on the downloaded planes"""
    from ada_ray_tracer_amd import scenes
    W, H = 40, 24
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=5)
    try:
        accum, moments, spp, aovs = frame_planes(art, backend, scenes.synthetic_scene(2000, 3), W, H, p, 2)
        var = torch.empty((H, W), dtype=torch.float32, device="cuda")
        out = backend.denoise_svgf_torch(accum, moments, spp // 4, **aovs, scale=1.0 / spp, variance_out=var)
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in aovs.items() if k != "alpha"}
        ref = S.denoise(accum.cpu().numpy(), moments.cpu().numpy(), 2, **h, scale=1.0 / spp, iterations=art.SVGF_ITERATIONS, sigma_color=art.SVGF_SIGMA_COLOR)
        assert spp == 8 and moments.any() and S.differ(out.cpu().numpy(), ref[0]) == 0 and S.differ(var.cpu().numpy(), ref[1]) == 0
        assert (var.cpu().numpy() > 0).any()
    finally:
        unbind(backend)


def test_quality_filtered_8_spp_is_closer_to_the_reference(art, backend):
    """the frame of tests/test_svgf_quality.py rendered and filtered on the GPU with the shipped defaults: RMS against the 1024-spp
    reference picture is lower after the filter than before"""
    p = art.Backend.pass_params(art.PT_MIS, False, Q.DEPTH, Q.SPP, seed=Q.SEED)
    try:
        accum, moments, spp, aovs = frame_planes(art, backend, Q.scene(), Q.W, Q.H, p, 1)
        out = backend.denoise_svgf_torch(accum, moments, spp, **aovs, scale=1.0 / spp)
        torch.cuda.synchronize()
        ref = Q.reference()
        before, after = Q.rms(accum.cpu().numpy() / F(spp), ref), Q.rms(out.cpu().numpy(), ref)
        print("RMS against 1024 spp: %.4f before, %.4f after" % (before, after))
        assert spp == Q.SPP and after < before
    finally:
        unbind(backend)
