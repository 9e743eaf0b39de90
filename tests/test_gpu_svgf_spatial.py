"""art_svgf_spatial_variance_device on the GPU against the numpy reference written from the header (tests/svgf_spatial_ref.py): bit
equality on the synthetic cases the host test shares, waves that mix short and long histories and waves that are long throughout, a side
stream with in-place output, the refusals that need a device, and the chain render -> feature buffers -> temporal -> spatial variance ->
variance-plane filter at one colour per frame, end to end."""
import ctypes as C

import numpy as np
import pytest

import svgf_spatial_ref as SP
import svgf_var_ref as V
import temporal_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_spatial(backend, hist, variance, in_place=False, **kw):
    """svgf_spatial_ref.spatial's signature through Backend.svgf_spatial_variance_torch"""
    H, W = hist.shape[1:3]
    kw = dict(dict(radius=3, min_history=4.0, sigma_depth=1.0, normal_log2=7), **kw)          # (the reference's defaults, not the package's)
    h, v = dev(np.asarray(hist, F)), dev(np.asarray(variance, F))
    out = v if in_place else torch.full((H, W), -7.0, dtype=torch.float32, device="cuda")
    got = backend.svgf_spatial_variance_torch(h, v, W, H, out=out, **kw)
    torch.cuda.synchronize()
    assert got is out and (in_place or SP.differ(v.cpu().numpy(), variance) == 0)          # (the input plane is only read)
    return got.cpu().numpy()


@pytest.mark.parametrize("radius", SP.RADII)
@pytest.mark.parametrize("size", SP.SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_reference(backend, size, radius):
    W, H = size
    for name, kw in SP.cases(W, H):
        ref = SP.spatial(radius=radius, **kw)
        assert SP.differ(gpu_spatial(backend, radius=radius, **kw), ref) == 0, name
        assert SP.differ(gpu_spatial(backend, radius=radius, in_place=True, **kw), ref) == 0, name + " (in place)"


def test_mixed_waves_and_waves_that_leave_early(backend):
    """83 x 41 is 6 x 3 tiles of 16 x 16, the last column and row partial.  A wave is a 16 x 4 strip of a tile.  (a) short pixels scattered
    one to a few strips: their waves take the divergent path with 63 lanes masked, every other wave is long throughout and leaves after
    the copy; (b) the left half short, the right half long: the strips that straddle x = 41 mix both; (c) whole strips short and whole strips long in turn, radius 1, no depth stop."""
    W, H = 83, 41
    X, Y = np.meshgrid(np.arange(W), np.arange(H))
    n = np.full((H, W), 8.0)
    n[(X % 23 == 5) & (Y % 9 == 2)] = 1.0
    for lengths, kw in ((n, dict(radius=3, min_history=4.0)), (np.where(X < 41, 1.0, 8.0), dict(radius=2, min_history=4.0)),
                        (np.where((X // 16 + Y // 4) % 2 == 0, 2.0, 8.0), dict(radius=1, min_history=4.0, sigma_depth=0.0))):
        h, v = SP.history(W, H, lengths, seed=9)
        ref = SP.spatial(h, v, **kw)
        long_ = (h[0, ..., 3] >= 4.0) & np.isfinite(v)
        assert 0 < long_.sum() < W * H and SP.differ(ref[long_], v[long_]) == 0 and SP.differ(ref[~long_], v[~long_]) > 0
        assert SP.differ(gpu_spatial(backend, h, v, **kw), ref) == 0


def test_side_stream_and_in_place(backend):
    """inputs copied on a torch side stream and the call enqueued there with no synchronisation in between, writing over its own input"""
    W, H = 70, 21
    X, Y = np.meshgrid(np.arange(W), np.arange(H))
    h, v = SP.history(W, H, np.where((X + Y) % 3 == 0, 1.0, 8.0), seed=4)
    ref = SP.spatial(h, v, radius=3, min_history=4.0, sigma_depth=1.0)
    hh, vh = torch.from_numpy(h).pin_memory(), torch.from_numpy(v).pin_memory()
    hd, vd = torch.zeros((3, H, W, 4), device="cuda"), torch.zeros((H, W), device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        hd.copy_(hh, non_blocking=True); vd.copy_(vh, non_blocking=True)
        got = backend.svgf_spatial_variance_torch(hd, vd, W, H, radius=3, min_history=4.0, sigma_depth=1.0, out=vd)
    st.synchronize()
    assert got is vd and SP.differ(vd.cpu().numpy(), ref) == 0 and torch.equal(hd.cpu(), hh)


def test_refusals(art, backend):
    W, H = 41, 25                                                    # N - 1 = 1024 pixels: the short planes below are whole 4 KiB pages
    L, N = backend.lib, W * H
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hist, vin = torch.zeros(12 * N, device="cuda"), torch.zeros(N, device="cuda")
    vout = torch.full((N,), 3.0, device="cuda")
    host = np.zeros(12 * N, F)
    good = [hist.data_ptr(), vin.data_ptr(), vout.data_ptr()]
    p = art.ArtSvgfSpatialParams(W, H, 3, 7, 4.0, 1.0)

    def refused(ptrs, text):
        rc = L.art_svgf_spatial_variance_device(C.byref(p), *ptrs, None)
        torch.cuda.synchronize()
        assert rc != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())
        assert bool((vout == 3.0).all())

    def but(i, v):
        q = list(good); q[i] = v
        return q
    refused(but(2, good[0]), "variance_out1f overlaps hist")
    refused(but(2, good[0] + 48 * N - 4), "variance_out1f overlaps hist")
    for i, (name, per) in enumerate((("hist", 48), ("variance_in1f", 4), ("variance_out1f", 4))):
        refused(but(i, host.ctypes.data), name + " is not device memory")
        short = C.c_void_p(None)                                     # an allocation of its own, too small by one pixel
        assert hip.hipMalloc(C.byref(short), (N - 1) * per) == 0
        try:
            refused(but(i, short.value), name + " is smaller than")
        finally:
            hip.hipFree(short)
    assert L.art_svgf_spatial_variance_device(C.byref(p), *good, None) == 0      # and the same arguments, unbroken, are accepted
    assert L.art_svgf_spatial_variance_device(C.byref(p), good[0], good[1], good[1], None) == 0
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_one_colour_per_frame(art, backend):
    """the four cameras of tests/temporal_quality.py's pan at 48 x 48, one colour per frame (no anti-aliasing, 1 spp): render with accum
    and moments bound -> feature buffers -> temporal -> spatial variance -> variance-plane filter, everything on the GPU with the
    shipped defaults; the same chain by the numpy references from the GPU's own render outputs gives the same bits in every plane.
    Then the quality the sweep recorded (profiles/svgf_spatial/quality.json): at the second frame, where every history is short, and at
    the last, the filtered picture WITH the call is closer to the 1024-spp reference than WITHOUT it by the asserted ratios."""
    import svgf_spatial_quality as Q
    accum = torch.zeros((Q.H, Q.W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((Q.H, Q.W, 2), dtype=torch.float32, device="cuda")
    rec = Q.shipped()
    refs = dict(zip((Q.SECOND, Q.LAST), Q.reference()))
    kw = dict(radius=art.SVGF_SPATIAL_RADIUS, min_history=art.SVGF_SPATIAL_MIN_HISTORY, sigma_depth=art.SVGF_SPATIAL_SIGMA_DEPTH)
    h_gpu, h_ref, prev, ratios = None, None, None, {}
    try:
        backend.upload_scene(Q.scene(0))
        backend.bind_accum(accum)
        backend.bind_moments(moments)
        for k in range(Q.FRAMES):
            p = art.Backend.pass_params(art.PT_MIS, False, Q.DEPTH, Q.SPP, seed=Q.SEED + k)
            backend.set_camera(*Q.camera(k))
            backend.resize(Q.W, Q.H)
            spp = backend.render_pass_device(p, 0)
            aovs = backend.render_aovs_torch(p, want=("albedo", "normal", "depth", "prim_index"))
            out, var, length, h_gpu = backend.temporal_torch(dict(aovs, color=accum, moments=moments), h_gpu, Q.camera(k), prev, spp, scale=1.0 / spp)
            var2 = backend.svgf_spatial_variance_torch(h_gpu, var, Q.W, Q.H)
            guides = dict(albedo=aovs["albedo"], normal=aovs["normal"], depth=aovs["depth"])
            filt = backend.denoise_svgf_torch(out, variance=var2, **guides)
            base = backend.denoise_svgf_torch(out, variance=var, **guides)
            torch.cuda.synchronize()
            hst = {n: v.cpu().numpy() for n, v in aovs.items()}
            r = T.temporal(accum.cpu().numpy(), moments.cpu().numpy(), spp, Q.camera(k), cam_prev=prev, hist=h_ref, normal=hst["normal"], depth=hst["depth"],
                           ids=hst["prim_index"], max_history=art.TEMPORAL_MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN,
                           scale=1.0 / spp)
            assert spp == Q.SPP == 1 and all(T.differ(a.cpu().numpy(), b) == 0 for a, b in zip((h_gpu, out, var, length), r)), "frame %d" % k
            rv = SP.spatial(r[0], r[2], **kw)
            assert SP.differ(var2.cpu().numpy(), rv) == 0, "frame %d" % k
            rf = V.denoise_var(r[1], rv, albedo=hst["albedo"], normal=hst["normal"], depth=hst["depth"], iterations=art.SVGF_ITERATIONS,
                               sigma_color=art.SVGF_SIGMA_COLOR)[0]
            assert T.differ(filt.cpu().numpy(), rf) == 0, "frame %d" % k
            hit = hst["depth"] > 0
            if k == 0:
                assert np.isinf(r[2]).all() and np.isfinite(rv[hit]).any()      # one colour: no variance anywhere before the call; some after it
            if k in refs:
                ratios[k] = Q.rms(filt.cpu().numpy(), refs[k]) / Q.rms(base.cpu().numpy(), refs[k])
            h_ref, prev = r[0], Q.camera(k)
        print("RMS with / without the call: second frame %.4f (bound %.4f), last frame %.4f (bound %.4f)"
              % (ratios[Q.SECOND], rec["asserted_ratio_second"], ratios[Q.LAST], rec["asserted_ratio_last"]))
        assert ratios[Q.SECOND] < rec["asserted_ratio_second"] and ratios[Q.LAST] < rec["asserted_ratio_last"]
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)
