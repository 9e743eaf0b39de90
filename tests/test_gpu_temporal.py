"""art_temporal_device and art_denoise_svgf_var_device on the GPU against the numpy references written from the header
(tests/temporal_ref.py, tests/svgf_var_ref.py): bit equality of every output plane and every history word on synthetic frames, a chain of
five frames, the optional planes, Backend.temporal_torch on a side stream, the refusals, and the chain render -> feature buffers ->
temporal -> variance-plane filter end to end."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as R
import svgf_ref as S
import svgf_var_ref as V
import temporal_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_temporal(art, backend, color, moments, n_colours, cam_cur, cam_prev=None, hist=None, normal=None, depth=None, ids=None, max_history=64,
                 depth_tol=0.05, normal_min=0.9, scale=1.0, want=(True, True, True)):
    """temporal_ref.temporal's signature through the C ABI: (hist_out, out, variance, length), None where not wanted"""
    H, W = color.shape[:2]
    d = [dev(np.asarray(color, F)), dev(np.asarray(moments, F)), dev(normal), dev(depth), dev(ids), dev(hist)]
    p = art.ArtTemporalParams()
    p.cur = backend.temporal_camera(cam_cur, W, H)
    if hist is not None:
        p.prev = backend.temporal_camera(cam_prev, hist.shape[2], hist.shape[1])
    p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = n_colours, max_history, scale, depth_tol, normal_min
    new = torch.full((3, H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    outs = [torch.full(s, -7.0, dtype=torch.float32, device="cuda") if w else None for s, w in zip(((H, W, 3), (H, W), (H, W)), want)]
    ptr = lambda x: None if x is None else x.data_ptr()
    rc = backend.lib.art_temporal_device(C.byref(p), *[ptr(x) for x in d], ptr(new), *[ptr(x) for x in outs], None)
    assert rc == 0, backend.lib.art_last_error().decode()
    torch.cuda.synchronize()
    return (new.cpu().numpy(),) + tuple(None if x is None else x.cpu().numpy() for x in outs)


def same(a, b):
    return all(T.differ(x, y) == 0 for x, y in zip(a, b))


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_reference(art, backend, size):
    W, H = size
    for name, kw in T.cases(W, H):
        assert same(gpu_temporal(art, backend, **kw), T.temporal(**kw)), name


def test_chain_of_five_frames(art, backend):
    got = T.run_chain(lambda **kw: gpu_temporal(art, backend, **kw), 64, 33)
    ref = T.run_chain(T.temporal, 64, 33)
    assert same(got, ref) and (ref[3] > 2).any()


def test_optional_outputs(art, backend):
    W, H = 13, 9
    kw = dict(T.cases(W, H))["pan"]
    ref = T.temporal(**kw)
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = gpu_temporal(art, backend, **kw, want=want)
        assert T.differ(got[0], ref[0]) == 0
        for k in range(3):
            assert (got[1 + k] is None) == (not want[k]) and (got[1 + k] is None or T.differ(got[1 + k], ref[1 + k]) == 0)


def test_temporal_torch_on_a_side_stream(art, backend):
    """Backend.temporal_torch: the dict of planes, inputs written on a torch side stream and the call enqueued there with no
    synchronisation in between; two frames, the second from the first's history"""
    W, H = 130, 3
    c0, c1 = T.cam(), T.cam((0.2, 0.0, -0.3), yaw=0.01)
    f0, f1 = T.frame(c0, W, H, seed=0), T.frame(c1, W, H, seed=1)
    kw = dict(max_history=16, depth_tol=0.05, normal_min=0.9, scale=0.5)
    r0 = T.temporal(n_colours=2, cam_cur=c0, **f0, **kw)
    r1 = T.temporal(n_colours=2, cam_cur=c1, cam_prev=c0, hist=r0[0], **f1, **kw)
    names = ("color", "moments", "normal", "depth", "ids")
    host = [[torch.from_numpy(np.ascontiguousarray(f[k])).pin_memory() for k in names] for f in (f0, f1)]
    d = [[torch.zeros_like(x, device="cuda") for x in hs] for hs in host]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        res, h = [], None
        for k, cam in enumerate((c0, c1)):
            for a, b in zip(d[k], host[k]):
                a.copy_(b, non_blocking=True)
            cur = dict(zip(("color", "moments", "normal", "depth", "prim_index"), d[k]), alpha=None, albedo=None)
            res.append(backend.temporal_torch(cur, h, cam, c0 if k else None, 2, **kw))
            h = res[-1][3]
    st.synchronize()
    for got, ref in zip(res, (r0, r1)):
        out, var, length, new = [x.cpu().numpy() for x in got]
        assert same((new, out, var, length), ref)
    assert (r1[3] > 2).any()


def test_refusals(art, backend):
    W, H = 41, 25                                                    # N - 1 = 1024 pixels: the short planes below are whole 4 KiB pages
    L = backend.lib
    N = W * H
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    t = lambda k, dt=torch.float32: torch.zeros(k * N, dtype=dt, device="cuda")
    color, mom, nrm, dep, ids, hin, hout, out, var, length = t(3), t(2), t(3), t(1), t(1, torch.int32), t(12), t(12), t(3), t(1), t(1)
    host = np.zeros(12 * N, F)
    good = [x.data_ptr() for x in (color, mom, nrm, dep, ids, hin, hout, out, var, length)]
    p = art.ArtTemporalParams()
    c = backend.temporal_camera(T.cam(), W, H)
    p.cur, p.prev = c, backend.temporal_camera(T.cam((0.1, 0, 0)), W, H)
    p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = 2, 16, 1.0, 0.05, 0.9

    def refused(ptrs, text):
        before = hout.clone()
        rc = L.art_temporal_device(C.byref(p), *ptrs, None)
        torch.cuda.synchronize()
        assert rc != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())
        assert torch.equal(hout, before)

    def but(i, v):
        q = list(good); q[i] = v
        return q
    refused(but(6, good[5]), "hist_in and hist_out overlap")
    refused(but(6, good[5] + 48 * N - 16), "hist_in and hist_out overlap")
    for i, (name, per) in enumerate((("color3f", 12), ("moments2f", 8), ("normal3f", 12), ("depth", 4), ("id", 4), ("hist_in", 48), ("hist_out", 48),
                                     ("out3f", 12), ("variance_out", 4), ("length_out", 4))):
        refused(but(i, host.ctypes.data), name + " is not device memory")
        short = C.c_void_p(None)                                     # an allocation of its own, too small by one pixel
        assert hip.hipMalloc(C.byref(short), (N - 1) * per) == 0
        try:
            refused(but(i, short.value), name + " is smaller than")
        finally:
            hip.hipFree(short)
    assert L.art_temporal_device(C.byref(p), *good, None) == 0              # and the same arguments, unbroken, are accepted
    assert L.art_temporal_device(C.byref(p), *good[:2], None, None, None, None, good[6], None, None, None, None) == 0
    torch.cuda.synchronize()
    # the variance-plane filter's pointer checks
    s = art.ArtSvgfParams(W, H, 2, 0, 7, 0, 1.0, 2.0, 1.0)
    for ptrs, text in (((good[0], host.ctypes.data, None, None, None, good[7], None), "variance1f is not device memory"),):
        assert L.art_denoise_svgf_var_device(C.byref(s), *ptrs, None) != 0 and text in L.art_last_error().decode()
    short = C.c_void_p(None)
    assert hip.hipMalloc(C.byref(short), (N - 1) * 4) == 0
    try:
        assert L.art_denoise_svgf_var_device(C.byref(s), good[0], short.value, None, None, None, good[7], None, None) != 0
        assert "variance1f is smaller than" in L.art_last_error().decode()
    finally:
        hip.hipFree(short)
    assert L.art_denoise_svgf_var_device(C.byref(s), good[0], good[8], None, None, None, good[7], None, None) == 0      # n_colours = 0 is ignored
    torch.cuda.synchronize()


# ---- the variance-plane filter --------------------------------------------------------------------------------------------------------
def run_var(backend, color, var, g, kw):
    H, W = color.shape[:2]
    vout = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
    out = backend.denoise_svgf_torch(dev(color), variance=dev(var), **{k: dev(v) for k, v in g.items()}, **kw, variance_out=vout)
    torch.cuda.synchronize()
    return out.cpu().numpy(), vout.cpu().numpy()


@pytest.mark.parametrize("size", S.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_variance_plane_filter_equals_its_reference(backend, size):
    W, H = size
    pl = R.planes(W, H)
    var = V.variance_plane(pl[0], W, H)
    for c in S.combos():
        if c[0] > 3 and size != (37, 23):
            continue                                    # iterations 5 and 8: on 37x23 only, as tests/test_gpu_svgf.py
        color, _, _, g, kw = S.combo_args(pl, c, W, H)
        got, ref = run_var(backend, color, var, g, kw), V.denoise_var(color, var, **g, **kw)
        assert S.differ(got[0], ref[0]) == 0 and S.differ(got[1], ref[1]) == 0, S.combo_id(c)


def test_variance_plane_from_the_moments_gives_the_moments_entrance(backend):
    """where the header says the two calls agree (scale a power of two, no demodulation): the same bits from both entry points; and
    the moments entrance is still its own reference's"""
    W, H = 65, 4
    color, albedo, normal, depth = R.planes(W, H)
    for nc in (2, 64):
        mom = S.moments_for(color, nc, W, H)
        kw = dict(iterations=2, scale=0.25, sigma_color=2.0)
        b = run_var(backend, color, V.variance_of(mom, nc), dict(normal=normal, depth=depth), kw)
        vout = torch.empty((H, W), dtype=torch.float32, device="cuda")
        a = backend.denoise_svgf_torch(dev(color), dev(mom), nc, normal=dev(normal), depth=dev(depth), **kw, variance_out=vout)
        ref = S.denoise(color, mom, nc, normal=normal, depth=depth, **kw)
        assert S.differ(a.cpu().numpy(), ref[0]) == 0 and S.differ(vout.cpu().numpy(), ref[1]) == 0
        assert S.differ(b[0], ref[0]) == 0 and S.differ(b[1], ref[1]) == 0


def test_cameras_at_rest_on_the_gpu(art, backend):
    """identical cameras: the fractional part is exactly 0, so the history is the previous record itself -- the length grows by n_cur per
    frame and stops at max_history, and the colour after two frames is the hand-computed mean, on the kernel's own outputs"""
    W, H = 13, 9
    c = T.cam()
    h, lengths = None, []
    for k in range(5):
        fr = T.frame(c, W, H, seed=k)
        h, out, var, n = gpu_temporal(art, backend, n_colours=2, cam_cur=c, cam_prev=c, hist=h, scale=0.5, max_history=7, **fr)
        hit = fr["depth"] > 0
        lengths.append(np.unique(n[hit]).tolist())
        assert (n[~hit] == 2).all() and np.isfinite(var[n >= 2]).all()
    assert lengths == [[2.0], [4.0], [6.0], [7.0], [7.0]]
    f0, f1 = T.frame(c, W, H, seed=0), T.frame(c, W, H, seed=1)
    h0 = gpu_temporal(art, backend, n_colours=2, cam_cur=c, scale=0.5, **f0)[0]
    out = gpu_temporal(art, backend, n_colours=2, cam_cur=c, cam_prev=c, hist=h0, scale=0.5, **f1)[1]
    hit = f1["depth"] > 0
    want = F(0.5) * (F(0.5) * f1["color"]) + F(0.5) * (F(0.5) * f0["color"])
    assert np.array_equal(out[hit], want[hit]) and np.array_equal(out[~hit], (F(0.5) * f1["color"])[~hit])


def test_quality_on_the_gpu(art, backend):
    """the frames of tests/test_temporal_quality.py rendered on the GPU at equal seeds (the camera moved by set_camera), accumulated and
    filtered with the shipped defaults: the RMS against the 1024-spp picture falls below the sweep's asserted ratio"""
    import temporal_quality as Q
    accum = torch.zeros((Q.H, Q.W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((Q.H, Q.W, 2), dtype=torch.float32, device="cuda")
    try:
        backend.upload_scene(Q.scene(0))
        backend.bind_accum(accum)
        backend.bind_moments(moments)
        h, prev = None, None
        for k in range(Q.FRAMES):
            p = art.Backend.pass_params(art.PT_MIS, False, Q.DEPTH, Q.SPP, seed=Q.SEED + k)
            backend.set_camera(*Q.camera(k))
            backend.resize(Q.W, Q.H)
            spp = backend.render_pass_device(p, 0)
            aovs = backend.render_aovs_torch(p, want=("albedo", "normal", "depth", "prim_index"))
            out, var, length, h = backend.temporal_torch(dict(aovs, color=accum, moments=moments), h, Q.camera(k), prev, spp, scale=1.0 / spp)
            prev = Q.camera(k)
        filt = backend.denoise_svgf_torch(out, variance=var, albedo=aovs["albedo"], normal=aovs["normal"], depth=aovs["depth"])
        torch.cuda.synchronize()
        ref = Q.reference()
        before, mid, after = Q.rms(accum.cpu().numpy() / F(spp), ref), Q.rms(out.cpu().numpy(), ref), Q.rms(filt.cpu().numpy(), ref)
        print("RMS against 1024 spp: %.4f last frame alone, %.4f accumulated, %.4f accumulated and filtered" % (before, mid, after))
        assert spp == Q.SPP and after < Q.bound(Q.shipped()) * before and mid < before
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_pan(art, backend):
    """the 48 x 48 scene at four cameras along a small pan, 2 colours each (8 spp with anti-aliasing): render with accum and moments bound
    -> feature buffers -> temporal -> variance-plane filter, everything on the GPU; the same chain by the numpy references from the GPU's
    own render outputs gives the same bits.  The camera moves by set_camera: the scene is uploaded once."""
    from ada_ray_tracer_amd import scenes
    W = H = 48
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=5)
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    eye = np.eye(4, dtype=F)
    h_gpu, h_ref, prev = None, None, None
    try:
        backend.upload_scene(scenes.synthetic_scene(2000, 3))
        backend.bind_accum(accum)
        backend.bind_moments(moments)
        for k in range(4):
            pos = (0.0 + 0.05 * k, 2.55, 12.5)
            backend.set_camera(pos, eye)
            backend.resize(W, H)
            spp = 0
            for _ in range(2):
                spp = backend.render_pass_device(p, spp)
            aovs = backend.render_aovs_torch(p, want=("albedo", "normal", "depth", "prim_index"))
            cam = (np.array(pos, F), eye)
            cur = dict(aovs, color=accum, moments=moments)
            out, var, length, h_gpu = backend.temporal_torch(cur, h_gpu, cam, prev, spp // 4, scale=1.0 / spp)
            vout = torch.empty((H, W), dtype=torch.float32, device="cuda")
            filt = backend.denoise_svgf_torch(out, variance=var, albedo=aovs["albedo"], normal=aovs["normal"], depth=aovs["depth"], variance_out=vout)
            torch.cuda.synchronize()
            hst = {n: v.cpu().numpy() for n, v in aovs.items()}
            r = T.temporal(accum.cpu().numpy(), moments.cpu().numpy(), spp // 4, cam, cam_prev=prev, hist=h_ref, normal=hst["normal"], depth=hst["depth"],
                           ids=hst["prim_index"], max_history=art.TEMPORAL_MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN,
                           scale=1.0 / spp)
            assert spp == 8 and same((h_gpu.cpu().numpy(), out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy()), r), "frame %d" % k
            rf = V.denoise_var(r[1], r[2], albedo=hst["albedo"], normal=hst["normal"], depth=hst["depth"], iterations=art.SVGF_ITERATIONS,
                               sigma_color=art.SVGF_SIGMA_COLOR)
            assert S.differ(filt.cpu().numpy(), rf[0]) == 0 and S.differ(vout.cpu().numpy(), rf[1]) == 0, "frame %d" % k
            hit = hst["depth"] > 0
            assert hit.mean() > 0.3 and (r[3][~hit] == 2).all()
            assert k == 0 or (r[3][hit] > 2).mean() > 0.5, "frame %d" % k      # most of what the camera sees found its history
            h_ref, prev = r[0], cam
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)
