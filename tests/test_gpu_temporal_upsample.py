"""art_temporal_upsample_device on the GPU against the numpy reference written from the header (tests/temporal_upsample_ref.py): bit
equality of every history word, output word and fallback byte on the shapes and cases the host test shares; the anchor (at equal sizes and
jitter 0 the call is art_temporal_device / art_temporal_motion_device); two chained calls on a caller's stream and the history handed to the
SVGF calls; the refusals (tests/golden/temporal_upsample_refusals.json); the jittered camera against camera_rays_torch; four jittered
24 x 24 passes of the test scene accumulated into 48 x 48 end to end; and the quality assertion of tests/test_temporal_upsample_quality.py."""
import ctypes as C

import numpy as np
import pytest

import temporal_motion_ref as TM
import temporal_ref as T
import temporal_upsample_ref as R
import temporal_upsample_refusals as RF
import test_temporal_upsample_reference_host as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_runner(backend):
    """temporal_upsample_ref.temporal_upsample's signature through Backend.temporal_upsample_torch: (hist_out, out, variance, length,
    fallback) as numpy arrays"""
    def run(lo_color, lo_moments, n_colours, cam_cur, cam_prev=None, hist=None, lo=None, hi=None, size=None, jitter=(0.0, 0.0), radius=1.0, min_confidence=0.25,
            max_history=64, depth_tol=0.05, normal_min=0.9, scale=1.0):
        lo = {k: dev(v) for k, v in (lo or {}).items() if v is not None}
        hi = {k: dev(v) for k, v in (hi or {}).items() if v is not None}
        c, m = dev(np.asarray(lo_color, F)), dev(np.asarray(lo_moments, F))
        out, var, length, new, fb = backend.temporal_upsample_torch(c, m, lo, hi, cam_cur, cam_prev, dev(hist), jitter=jitter, n_colours=n_colours, scale=scale,
                                                                    radius=radius, min_confidence=min_confidence, max_history=max_history, depth_tol=depth_tol,
                                                                    normal_min=normal_min, size=size, want_fallback=True)
        torch.cuda.synchronize()
        assert R.differ(c.cpu().numpy(), np.asarray(lo_color, F)) == 0      # (the input plane is only read)
        return new.cpu().numpy(), out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy(), fb.cpu().numpy()
    return run


def differences(want, got):
    return [R.differ(a, b) for a, b in zip(want[:5], got)]


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_kernels_equal_the_reference(backend, shape):
    run = gpu_runner(backend)
    wrong = []
    for name, kw, ref in R.reference_results(shape):
        d = differences(ref, run(**kw))
        if any(d):
            wrong.append("%s: words that differ in (hist_out, out3f, variance, length), bytes in fallback: %s" % (name, d))
    assert not wrong, "\n".join(wrong)


def test_every_line_of_step_c_on_the_gpu(backend):
    """the frame that takes all five lines of step C: the reference's own output visits each (so the case cannot pass by leaving one out)
    and the kernel gives its bits"""
    shape = R.SHAPES[4]
    name, kw, ref = [r for r in R.reference_results(shape) if r[0] == "five_branches"][0]
    assert sorted(np.unique(ref[5])) == [0, 1, 2, 3, 4]
    assert not any(differences(ref, gpu_runner(backend)(**kw)))


def test_optional_outputs_may_be_null(art, backend):
    shape = W, H, LW, LH = R.SHAPES[3]
    name, kw, ref = [r for r in R.reference_results(shape) if r[0] == "jitter1_rest"][0]
    TU = art.temporal_upsample
    p = TU.params_struct()()
    p.t.cur = backend.temporal_camera(kw["cam_cur"], W, H)
    p.t.prev = backend.temporal_camera(kw["cam_prev"], W, H)
    p.t.n_colours, p.t.max_history, p.t.scale, p.t.depth_tol, p.t.normal_min = kw["n_colours"], kw["max_history"], kw["scale"], kw["depth_tol"], kw["normal_min"]
    p.lo_width, p.lo_height, p.radius, p.min_confidence = LW, LH, kw["radius"], kw["min_confidence"]
    p.jitter[0], p.jitter[1] = kw["jitter"]
    keep = [dev(kw["lo_color"]), dev(kw["lo_moments"]), dev(kw["hist"])] + [dev(kw[s][k]) for s in ("lo", "hi") for k in ("normal", "depth", "id")]
    lo = TU.ArtTemporalUpsampleGuides(*[x.data_ptr() for x in keep[3:6]], None)
    hi = TU.ArtTemporalUpsampleGuides(*[x.data_ptr() for x in keep[6:9]], None)
    new = torch.full((3, H, W, 4), -7.0, device="cuda")
    rc = backend.lib.art_temporal_upsample_device(C.byref(p), keep[0].data_ptr(), keep[1].data_ptr(), C.byref(lo), C.byref(hi), keep[2].data_ptr(), new.data_ptr(),
                                                  None, None, None, None, None)
    torch.cuda.synchronize()
    assert rc == 0, backend.lib.art_last_error().decode()
    assert R.differ(new.cpu().numpy(), ref[0]) == 0


# ---- the anchor -----------------------------------------------------------------------------------------------------------------------
def test_at_equal_sizes_and_jitter_0_the_call_is_art_temporal_device(art, backend):
    """every output and history word of art_temporal_device (with a motion plane: art_temporal_motion_device) on the same planes"""
    run, ran = gpu_runner(backend), 0
    for name, kw in T.cases(13, 9) + TM.cases(13, 9) + T.cases(64, 33):
        if not (P.finite_case(kw) and P.own_tap_counts(kw)):
            continue
        H, W = kw["color"].shape[:2]
        cur = dict(color=dev(kw["color"]), moments=dev(kw["moments"]), normal=dev(kw.get("normal")), depth=dev(kw.get("depth")), prim_index=dev(kw.get("ids")))
        out, var, length, new = backend.temporal_torch(cur, dev(kw["hist"]), kw["cam_cur"], kw["cam_prev"], kw["n_colours"], max_history=kw["max_history"],
                                                       depth_tol=kw["depth_tol"], normal_min=kw["normal_min"], scale=kw["scale"], motion=dev(kw.get("motion")))
        torch.cuda.synchronize()
        want = (new.cpu().numpy(), out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy())
        for radius in (1.0, 0.37):
            got = run(**P.as_upsample(kw, radius, 0.25))
            assert not any(R.differ(a, b) for a, b in zip(want, got[:4])) and not got[4].any(), (name, radius)
        ran += 1
    assert ran >= 30


# ---- a chain on the caller's stream, and the history in the SVGF calls -------------------------------------------------------------------
def test_two_chained_calls_on_a_side_stream_feed_the_svgf_calls(art, backend):
    """the planes copied on a torch side stream and both calls enqueued there with no synchronisation in between: the second call's history
    and outputs are the reference's bits; hist_out and variance_out are accepted by art_svgf_spatial_variance_device and
    art_denoise_svgf_var_device as art_temporal_device's are, and give those calls' reference bits"""
    import svgf_spatial_ref as SS
    import svgf_var_ref as V
    shape = W, H, LW, LH = R.SHAPES[3]
    camr, top = T.cam(), R.bound(*shape)
    fr = [R.frames(W, H, LW, LH, camr, R.JITTERS[k + 1], 7 + k) for k in range(2)]
    kw = dict(n_colours=R.NC, scale=1.0 / R.NC, max_history=16, depth_tol=0.05, normal_min=0.9, min_confidence=0.25, radius=min(1.5, top))
    r0 = R.temporal_upsample(fr[0][0], fr[0][1], cam_cur=camr, lo=fr[0][2], hi=fr[0][3], jitter=R.JITTERS[1], **kw)
    r1 = R.temporal_upsample(fr[1][0], fr[1][1], cam_cur=camr, cam_prev=camr, hist=r0[0], lo=fr[1][2], hi=fr[1][3], jitter=R.JITTERS[2], **kw)
    pin = lambda x: torch.from_numpy(np.ascontiguousarray(x)).pin_memory()
    host = [(pin(c), pin(m), {k: pin(v) for k, v in lo.items()}, {k: pin(v) for k, v in hi.items()}) for c, m, lo, hi in fr]
    on_gpu = [(torch.zeros_like(c, device="cuda"), torch.zeros_like(m, device="cuda"), {k: torch.zeros_like(v, device="cuda") for k, v in lo.items()},
               {k: torch.zeros_like(v, device="cuda") for k, v in hi.items()}) for c, m, lo, hi in host]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for (hc, hm, hlo, hhi), (c, m, lo, hi) in zip(host, on_gpu):
            c.copy_(hc, non_blocking=True); m.copy_(hm, non_blocking=True)
            for k in lo:
                lo[k].copy_(hlo[k], non_blocking=True); hi[k].copy_(hhi[k], non_blocking=True)
        h = None
        for k, (c, m, lo, hi) in enumerate(on_gpu):
            out, var, length, h, fb = backend.temporal_upsample_torch(c, m, lo, hi, camr, camr, h, jitter=R.JITTERS[k + 1], want_fallback=True, **kw)
        var2 = backend.svgf_spatial_variance_torch(h, var, W, H)
        filt = backend.denoise_svgf_torch(out, variance=var2, normal=hi["normal"], depth=hi["depth"])
    side.synchronize()
    got = (h.cpu().numpy(), out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy(), fb.cpu().numpy())
    assert not any(differences(r1, got)) and (r1[3] > r0[3]).any()
    want_var = SS.spatial(r1[0], r1[2], radius=art.SVGF_SPATIAL_RADIUS, min_history=art.SVGF_SPATIAL_MIN_HISTORY, sigma_depth=art.SVGF_SPATIAL_SIGMA_DEPTH,
                                   normal_log2=7)
    assert R.differ(var2.cpu().numpy(), want_var) == 0
    want_filt = V.denoise_var(r1[1], want_var, normal=fr[1][3]["normal"], depth=fr[1][3]["depth"], iterations=art.SVGF_ITERATIONS, sigma_color=art.SVGF_SIGMA_COLOR)[0]
    assert R.differ(filt.cpu().numpy(), want_filt) == 0


def test_fallback_bytes_select_the_pixels_of_a_masked_pass(backend):
    shape = W, H, LW, LH = R.SHAPES[4]
    name, kw, ref = [r for r in R.reference_results(shape) if r[0] == "five_branches"][0]
    fb = ref[4]
    assert (fb == 1).any() and (fb == 2).any()
    gfb = dev(gpu_runner(backend)(**kw)[4])
    backend.resize(W, H)
    pixels, count = backend.compact_mask_torch(gfb)
    torch.cuda.synchronize()
    n = int(count.item())
    assert n == int((fb != 0).sum())
    assert sorted(pixels[:n].cpu().numpy().view(np.uint32).tolist()) == np.flatnonzero(fb.reshape(-1)).tolist()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_fixture(art, backend):
    """every case of tests/golden/temporal_upsample_refusals.json over device planes: refused with its message and nothing written; then the
    good call is accepted and writes every output"""
    frame, cases = RF.load()
    sizes = RF.plane_bytes(frame)
    offsets, at = {}, 0
    for k in RF.PLANES:
        offsets[k] = at
        at += (sizes[k] + 255) // 256 * 256
    arena = torch.full((at + 4096,), 0x5a, dtype=torch.uint8, device="cuda")
    base = {k: arena.data_ptr() + offsets[k] for k in RF.PLANES}
    outputs = ("hist_out", "out3f", "variance_out", "length_out", "fallback1b")
    host = np.zeros(sizes["hist_in"] // 4, F)
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
        return all(bool((arena[offsets[k]:offsets[k] + sizes[k]] == 0x5a).all()) for k in outputs)
    try:
        for case in cases:
            RF.check(art, backend.lib, frame, case, base, host=host.ctypes.data, short=short)
            assert untouched(), case["name"]
    finally:
        torch.cuda.synchronize()
        for p in held:
            hip.hipFree(p)
    rc, text = RF.call(art, backend.lib, frame, dict(name="good"), base)
    torch.cuda.synchronize()
    assert rc == 0, text
    for k in outputs:
        assert not bool((arena[offsets[k]:offsets[k] + sizes[k]] == 0x5a).all()), k
    # and from Python: bad tensors before any call, the library's refusals as ArtError
    W, H, LW, LH = frame
    lc, lm = torch.zeros((LH, LW, 3), device="cuda"), torch.zeros((LH, LW, 2), device="cuda")
    cam = T.cam()
    with pytest.raises(art.ArtError, match="GPU tensor"):
        backend.temporal_upsample_torch(lc, lm.cpu(), {}, {}, cam, size=(W, H))
    with pytest.raises(art.ArtError, match="radius must be inside"):
        backend.temporal_upsample_torch(lc, lm, {}, {}, cam, size=(W, H), radius=2.0)
    with pytest.raises(art.ArtError, match="min_confidence must be inside"):
        backend.temporal_upsample_torch(lc, lm, {}, {}, cam, size=(W, H), min_confidence=0.0)


# ---- the jittered camera ----------------------------------------------------------------------------------------------------------------
def test_jittered_camera_traces_the_jittered_grid(art, backend):
    """after set_camera(jittered_camera(...)) at 24 x 24, camera_rays_torch gives the directions normalize(M (r + j)) of the lo grid moved by
    the jitter, within 1e-6 absolute (a few binary32 roundings of unit vectors) of that expression in binary64; the camera is put back"""
    import temporal_quality as Q
    LW = LH = 24
    pos, m = Q.camera(1)
    rng = np.random.default_rng(2)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    turned = np.eye(4, dtype=F)
    turned[:3, :3] = (0.9 * np.eye(3) + 0.1 * q).astype(F)              # not orthonormal: the shear is a statement about any 3 x 3
    p = art.Backend.pass_params(art.PT_MIS, False, Q.DEPTH, 1, seed=Q.SEED)
    backend.upload_scene(Q.scene(1))
    backend.resize(LW, LH)
    try:
        for mat in (m, turned):
            for jit in [tuple(float(v) for v in j) for j in art.temporal_upsample.jitter_sequence(3)] + [(R.NEAR, -R.NEAR)]:
                backend.set_camera(pos, art.temporal_upsample.jittered_camera(mat, LW, jit))
                o, d = backend.camera_rays_torch(p)
                torch.cuda.synchronize()
                X, Y = np.meshgrid(np.arange(LW) + 0.5 - LW / 2.0, np.arange(LH) + 0.5 - LH / 2.0)
                r = np.stack([X + jit[0], Y + jit[1], np.full_like(X, -float(LW))], -1).reshape(-1, 3)
                want = r @ mat[:3, :3].astype(np.float64).T
                want /= np.linalg.norm(want, axis=-1, keepdims=True)
                err = np.abs(d.cpu().numpy().astype(np.float64) - want).max()
                print("jitter %s: max abs error of the directions %.3g" % (jit, err))
                assert err <= 1e-6, (jit, err)
                assert (o.cpu().numpy() == np.asarray(pos, F)).all()
    finally:
        backend.set_camera(pos, m)
    o, d = backend.camera_rays_torch(p)
    torch.cuda.synchronize()
    X, Y = np.meshgrid(np.arange(LW) + 0.5 - LW / 2.0, np.arange(LH) + 0.5 - LH / 2.0)
    r = np.stack([X, Y, np.full_like(X, -float(LW))], -1).reshape(-1, 3)
    assert np.abs(d.cpu().numpy() - r / np.linalg.norm(r, axis=-1, keepdims=True)).max() <= 1e-6      # restored


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_four_jittered_passes_into_48x48(art, backend):
    """INTEGRATION.md section 6l's loop on tests/temporal_quality.py's scene: per frame the jittered camera, a 24 x 24 pass with accum and
    moments bound, the lo feature buffers, the camera back, the hi feature buffers at 48 x 48, the call.  Two frames at one camera and two at
    the next, so the history is also reprojected.  Every frame equals the numpy reference fed with the same planes read back, bit for bit;
    the history grows and the last frame is a picture."""
    import temporal_quality as Q
    LW = LH = 24
    TU = art.temporal_upsample
    accum = torch.zeros((LH, LW, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((LH, LW, 2), dtype=torch.float32, device="cuda")
    names = ("normal", "depth", "prim_index")
    jit = TU.jitter_sequence(4)
    top = R.bound(Q.W, Q.H, LW, LH)
    h_gpu, h_ref, prev = None, None, None
    try:
        backend.upload_scene(Q.scene(0))
        for k in range(4):
            cam = Q.camera(k // 2)
            j = (float(jit[k][0]), float(jit[k][1]))
            p = art.Backend.pass_params(art.PT_MIS, False, Q.DEPTH, Q.SPP, seed=Q.SEED + k)
            backend.set_camera(cam[0], TU.jittered_camera(cam[1], LW, j))
            backend.bind_accum(accum)
            backend.bind_moments(moments)
            backend.resize(LW, LH)
            spp = backend.render_pass_device(p, 0)
            lo = backend.render_aovs_torch(p, want=names)
            backend.bind_accum(None)
            backend.bind_moments(None)
            backend.set_camera(*cam)
            backend.resize(Q.W, Q.H)
            hi = backend.render_aovs_torch(p, want=names)
            lo, hi = dict(lo, id=lo["prim_index"]), dict(hi, id=hi["prim_index"])
            out, var, length, h_gpu, fb = backend.temporal_upsample_torch(accum, moments, lo, hi, cam, prev, h_gpu, jitter=j, n_colours=spp, scale=1.0 / spp,
                                                                          want_fallback=True)
            torch.cuda.synchronize()
            ref = R.temporal_upsample(accum.cpu().numpy(), moments.cpu().numpy(), spp, cam, prev, h_ref, {g: lo[g].cpu().numpy() for g in R.GUIDES},
                                      {g: hi[g].cpu().numpy() for g in R.GUIDES}, jitter=j, radius=min(TU.TEMPORAL_UPSAMPLE_RADIUS, top),
                                      min_confidence=TU.TEMPORAL_UPSAMPLE_MIN_CONFIDENCE, max_history=art.TEMPORAL_MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL,
                                      normal_min=art.TEMPORAL_NORMAL_MIN, scale=1.0 / spp)
            got = (h_gpu.cpu().numpy(), out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy(), fb.cpu().numpy())
            assert spp == Q.SPP and not any(differences(ref, got)), "frame %d: %s" % (k, differences(ref, got))
            assert k == 0 or (ref[3] > lengths).mean() > 0.5, "frame %d" % k      # most pixels found their history and grew
            lengths, h_ref, prev = ref[3], ref[0], cam
        assert tuple(out.shape) == (Q.H, Q.W, 3) and len(np.unique(ref[1].reshape(-1, 3), axis=0)) > 256 and (ref[4] == 0).mean() > 0.9
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)


def test_accumulated_jittered_frames_beat_one_frame_and_plain_accumulation(art, backend):
    """the assertions of tests/test_temporal_upsample_quality.py of the kernels, on the same inputs: A < ((1 + r) / 2) * B and likewise
    against C, with the setting and the ratios the sweep recorded (profiles/temporal_upsample/quality.json)"""
    import test_temporal_upsample_quality as TQ
    TQ.accumulation_beats_its_neighbours(gpu_runner(backend), art)
