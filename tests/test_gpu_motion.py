"""The motion plane (art_render_aovs_motion_device) and the temporal call that uses it (art_temporal_motion_device) on the GPU against the
numpy references written from the header (tests/motion_ref.py, tests/temporal_motion_ref.py): bit equality on a flat scene after a refit
and after a rebuild, on instanced scenes after a move, on the synthetic temporal cases, the refusals one by one, a caller's stream, and
four frames of a translating mesh end to end.  The hits the plane's reference is fed are art_trace_rays' of the same camera rays, the
way tests/test_gpu_aov.py holds the other planes."""
import ctypes as C

import numpy as np
import pytest

import motion_ref as M
import temporal_motion_ref as TM
import temporal_ref as T
import test_gpu_aov as aov

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
ALL = aov.ALL


def gpu(a, dt=F):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def params(art, aa):
    return art.Backend.pass_params(art.RT_DEBUG, aa, 0, 0, seed=12345, layout=art.LAYOUT_ADA_XY)


def zero_words(t):
    return bool((aov.words(t) == 0).all())


# ---- flat scene ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat():
    """Cornell box, three spheres and a CLOSEST soup of 300 triangles; its vertices at three poses: a third of the triangles stay where
    they are, the others translate and wobble"""
    from ada_ray_tracer_amd import scenes
    sd = scenes.synthetic_scene(300, 3)
    pos, nrm, idx, _, matid = sd._mesh_arrays[-1]
    rng = np.random.default_rng(3)
    poses = [np.ascontiguousarray(pos, F)]
    for k in (1, 2):
        d = (np.array([0.13, -0.05, 0.21]) * k + rng.normal(0, 0.02, pos.shape)).astype(F)
        d.reshape(-1, 3, 3)[::3] = 0                  # (a de-indexed soup: three vertices per triangle)
        poses.append((pos + d).astype(F))
    return dict(sd=sd, idx=np.asarray(idx, np.int32).reshape(-1, 3), poses=poses)


def flat_reference(art, backend, flat, W, H, aa, cur, prev):
    """the eight planes of the scene as it lies on the GPU: art_trace_rays' hits of the camera rays through the header's arithmetic"""
    sd = flat["sd"]
    want, raw = aov.reference(art, backend, sd, W, H, aa)
    assert not ((raw[:, :, 1] == 1) & (raw[:, :, 2] == 2) & (raw[:, :, 3] >= flat["idx"].shape[0])).any()      # no REFERENCE_BF mesh: type 2 is the soup
    dirs = aov.camera_dirs(sd.desc, W, H, aa)
    want["motion"] = M.from_hits(raw, dirs, np.array(list(sd.desc.cam_pos), F), idx=flat["idx"], cur=cur, prev=prev).reshape(H, W, 3)
    return want, raw


@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("frame", [(48, 48), (37, 23)])
def test_flat_scene_after_a_refit_and_after_a_rebuild(art, backend, flat, frame, aa):
    W, H = frame
    p0, p1, p2 = flat["poses"]
    backend.upload_scene(flat["sd"]); backend.resize(W, H)
    backend.set_option("query_slice", 700)                       # several slices, the boundaries inside rows
    try:
        p = params(art, aa)
        # before any refit there is no plan: the call builds it
        first = backend.render_aovs_torch_motion(p, ALL, cur_pos=gpu(p0), prev_pos=gpu(p0))
        assert zero_words(first["motion"])
        backend.refit_torch(gpu(p1))
        got = backend.render_aovs_torch_motion(p, ALL, cur_pos=gpu(p1), prev_pos=gpu(p0))
        old = backend.render_aovs_torch(p, ALL)
        only = backend.render_aovs_torch_motion(p, (), cur_pos=gpu(p1), prev_pos=gpu(p0))
        none = backend.render_aovs_torch_motion(p, ("depth",))
        same = backend.render_aovs_torch_motion(p, ("depth",), cur_pos=gpu(p1), prev_pos=gpu(p1))
        torch.cuda.synchronize()
        want, raw = flat_reference(art, backend, flat, W, H, aa, p1, p0)
        aov.assert_planes(got, old, what="the seven planes of the new call")
        aov.assert_planes(got, want, what="after a refit")
        assert M.differ(got["motion"].cpu().numpy(), want["motion"]) == 0
        assert set(only) == {"motion"} and M.differ(only["motion"].cpu().numpy(), want["motion"]) == 0
        assert zero_words(none["motion"]) and zero_words(same["motion"])
        mo = want["motion"]
        on_mesh = want["prim_type"] == 2
        assert on_mesh.sum() > 30 and (mo[on_mesh] != 0).any() and np.isfinite(mo).all()
        if not aa:
            assert (mo[~on_mesh] == 0).all()
        # a rebuild drops the plan; the next call builds it again
        backend.rebuild_torch(gpu(p2))
        got = backend.render_aovs_torch_motion(p, ALL, cur_pos=gpu(p2), prev_pos=gpu(p1))
        torch.cuda.synchronize()
        want, _ = flat_reference(art, backend, flat, W, H, aa, p2, p1)
        aov.assert_planes(got, want, what="after a rebuild")
        assert M.differ(got["motion"].cpu().numpy(), want["motion"]) == 0 and (want["motion"] != 0).any()
    finally:
        backend.set_option("query_slice", 1 << 24)
    backend.synchronize()


def test_a_call_between_two_passes_changes_nothing(art, backend, flat):
    W, H = 48, 48
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=5)
    p0, p1 = flat["poses"][:2]
    backend.upload_scene(flat["sd"])

    def two_passes(between):
        backend.resize(W, H)
        _, _, spp = backend.render_pass(p, 0, want_accum=False)
        between()
        accum, _, spp = backend.render_pass(p, spp)
        st, sg = backend.stats(), backend.stage_stats()
        return (aov.words(accum).copy(), spp, (st.rays, st.samples, st.trace_launches, st.lost_paths),
                (sg.shade_launches, sg.batches, list(sg.items_in), list(sg.items_out)), backend.camera_rays_traced())

    plain = two_passes(lambda: None)
    seen = []
    with_call = two_passes(lambda: seen.append(backend.render_aovs_torch_motion(params(art, True), ALL, cur_pos=gpu(p0), prev_pos=gpu(p1))))
    assert plain[1] == with_call[1] == 8 and np.array_equal(plain[0], with_call[0])
    assert plain[2:] == with_call[2:]
    assert (seen[0]["motion"] != 0).any()


# ---- instanced scenes ---------------------------------------------------------------------------------------------------------------
def moved_matrices(m0):
    """instance j: j % 3 == 0 translated, 1 rotated about y and shifted, 2 where it was"""
    m1 = m0.copy()
    c, s = np.cos(0.2), np.sin(0.2)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    for j in range(m0.shape[0]):
        a = m0[j].reshape(3, 4).astype(np.float64)
        if j % 3 == 0:
            a[:, 3] += [0.21, -0.08, 0.15]
        elif j % 3 == 1:
            a[:, :3] = R @ a[:, :3]; a[:, 3] += [-0.05, 0.1, 0.0]
        m1[j] = a.astype(F).reshape(12)
    return m1


@pytest.mark.parametrize("n_inst", [1, 3, 70])
def test_instanced_scene_after_a_move(art, backend, n_inst):
    from ada_ray_tracer_amd import scenes
    W, H = 48, 48
    sd = scenes.instanced_scene(n_inst, 200)
    m0 = np.array([list(sd.desc.instances[i].m) for i in range(n_inst)], F)
    m1 = moved_matrices(m0)
    backend.upload_scene(sd); backend.resize(W, H)
    cam = np.array(list(sd.desc.cam_pos), F)
    for aa in (True, False):
        p = params(art, aa)
        still = backend.render_aovs_torch_motion(p, ("depth",), prev_matrices=gpu(m0))
        assert zero_words(still["motion"]), "the uploaded matrices against themselves"
    backend.move_instances_torch(gpu(m1))
    tl = backend.export_two_level()
    inst = tl["inst"][:n_inst].view(F)
    kw = dict(m_cur=inst[:, :12].copy(), minv_cur=inst[:, 12:24].copy(), prev_m=m0, inst_shift=tl["inst_shift"])
    assert np.array_equal(kw["m_cur"].view(np.uint32), m1.view(np.uint32))
    for aa in (True, False):
        p = params(art, aa)
        got = backend.render_aovs_torch_motion(p, ALL, prev_matrices=gpu(m0))
        none = backend.render_aovs_torch_motion(p, (), prev_matrices=None)
        torch.cuda.synchronize()
        want, raw = aov.reference(art, backend, sd, W, H, aa)
        dirs = aov.camera_dirs(sd.desc, W, H, aa)
        ref = M.from_hits(raw, dirs, cam, **kw).reshape(H, W, 3)
        aov.assert_planes(got, want, what="instanced, %d" % n_inst)
        assert M.differ(got["motion"].cpu().numpy(), ref) == 0, (n_inst, aa)
        assert zero_words(none["motion"])
        tri = (raw[:, :, 1] == 1) & (raw[:, :, 2] == 2)
        unmoved = (~tri | ((raw[:, :, 3] >> tl["inst_shift"]) % 3 == 2)).all(0).reshape(H, W)
        assert (ref[unmoved] == 0).all()
        if n_inst > 1:
            assert (ref != 0).any() and tri.any()
    backend.synchronize()


# ---- the temporal kernel ------------------------------------------------------------------------------------------------------------
def gpu_temporal(art, backend, color, moments, n_colours, cam_cur, cam_prev=None, hist=None, normal=None, depth=None, ids=None, max_history=64,
                 depth_tol=0.05, normal_min=0.9, scale=1.0, motion=None, entry="art_temporal_motion_device"):
    H, W = color.shape[:2]
    dev = lambda x, dt=F: None if x is None else gpu(x, dt)
    d = [dev(color), dev(moments), dev(normal), dev(depth), dev(ids, np.int32)]
    mo, hi = dev(motion), dev(hist)
    p = art.ArtTemporalParams()
    p.cur = backend.temporal_camera(cam_cur, W, H)
    if hist is not None:
        p.prev = backend.temporal_camera(cam_prev, hist.shape[2], hist.shape[1])
    p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = n_colours, max_history, scale, depth_tol, normal_min
    new = torch.full((3, H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    outs = [torch.full(s, -7.0, dtype=torch.float32, device="cuda") for s in ((H, W, 3), (H, W), (H, W))]
    ptr = lambda x: None if x is None else x.data_ptr()
    if entry == "art_temporal_motion_device":
        rc = backend.lib.art_temporal_motion_device(C.byref(p), *[ptr(x) for x in d], ptr(mo), ptr(hi), ptr(new), *[ptr(x) for x in outs], None)
    else:
        rc = backend.lib.art_temporal_device(C.byref(p), *[ptr(x) for x in d], ptr(hi), ptr(new), *[ptr(x) for x in outs], None)
    assert rc == 0, backend.lib.art_last_error().decode()
    torch.cuda.synchronize()
    return (new.cpu().numpy(),) + tuple(x.cpu().numpy() for x in outs)


def same(a, b):
    return all(T.differ(x, y) == 0 for x, y in zip(a, b))


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: "%dx%d" % s)
def test_temporal_motion_kernel_equals_the_reference(art, backend, size):
    W, H = size
    for name, kw in TM.cases(W, H):
        assert same(gpu_temporal(art, backend, **kw), TM.temporal(**kw)), name


def test_without_motion_the_new_entry_is_the_old_one(art, backend):
    W, H = 64, 33
    for name, kw in T.cases(W, H):
        new, old = gpu_temporal(art, backend, **kw), gpu_temporal(art, backend, **kw, entry="art_temporal_device")
        assert same(new, old) and same(new, T.temporal(**kw)), name


def test_temporal_torch_with_motion_on_a_side_stream(art, backend):
    W, H = 130, 3
    c0 = T.cam()
    f0, f1 = T.frame(c0, W, H, seed=0), T.frame(c0, W, H, seed=1)
    mo = TM.pixel_shift(c0, f1, 1.5, 0.0)
    kw = dict(max_history=16, depth_tol=0.05, normal_min=0.9, scale=0.5)
    r0 = T.temporal(n_colours=2, cam_cur=c0, **f0, **kw)
    r1 = TM.temporal(n_colours=2, cam_cur=c0, cam_prev=c0, hist=r0[0], motion=mo, **f1, **kw)
    names = ("color", "moments", "normal", "depth", "ids")
    host = [[torch.from_numpy(np.ascontiguousarray(f[k])).pin_memory() for k in names] for f in (f0, f1)]
    host_mo = torch.from_numpy(mo).pin_memory()
    d = [[torch.zeros_like(x, device="cuda") for x in hs] for hs in host]
    d_mo = torch.zeros_like(host_mo, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        res, h = [], None
        for k in range(2):
            for a, b in zip(d[k], host[k]):
                a.copy_(b, non_blocking=True)
            d_mo.copy_(host_mo, non_blocking=True)
            cur = dict(zip(("color", "moments", "normal", "depth", "prim_index"), d[k]))
            res.append(backend.temporal_torch(cur, h, c0, c0 if k else None, 2, motion=d_mo if k else None, **kw))
            h = res[-1][3]
    st.synchronize()
    for got, ref in zip(res, (r0, r1)):
        out, var, length, new = [x.cpu().numpy() for x in got]
        assert same((new, out, var, length), ref)
    assert (r1[3] > 2).any() and (r1[3] == 2).any()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_motion_plane(art, backend, flat):
    from ada_ray_tracer_amd import scenes
    W, H = 41, 25                                                    # N - 1 = 1024 pixels: a plane short by one pixel is whole 4 KiB pages
    L = backend.lib
    N = W * H
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    p0 = flat["poses"][0]
    nv = p0.shape[0]
    backend.upload_scene(flat["sd"]); backend.resize(W, H)
    p = params(art, True)
    cur, prev, mats = gpu(p0), gpu(flat["poses"][1]), gpu(np.zeros((4, 12), F))
    motion = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
    depth = torch.full((H, W), -7.0, dtype=torch.float32, device="cuda")
    buf = art.ArtAovBuffers(); buf.depth = depth.data_ptr()
    host = np.zeros(3 * max(N, nv), F)
    before = backend.render_aovs_torch(p, ALL)

    def src(cur_p=cur.data_ptr(), prev_p=prev.data_ptr(), n=nv, m=None, ni=0):
        return art.ArtMotionSource(cur_p, prev_p, n, m, ni)

    def refused(s, text, mo=motion.data_ptr()):
        rc = L.art_render_aovs_motion_device(C.byref(p), C.byref(buf), None if s is None else C.byref(s), mo, None)
        torch.cuda.synchronize()
        msg = L.art_last_error().decode()
        assert rc != 0 and text in msg, (text, msg)
        assert bool((motion == -7.0).all()) and bool((depth == -7.0).all())

    refused(None, "null src")
    refused(src(prev_p=None), "both be given or both be null")
    refused(src(cur_p=None), "both be given or both be null")
    refused(src(n=nv - 1), "nverts %d differs from the uploaded mesh's %d" % (nv - 1, nv))
    refused(src(m=mats.data_ptr(), ni=4), "the scene is not instanced")
    refused(src(None, None, 0, mats.data_ptr(), 4), "the scene is not instanced")
    refused(src(cur_p=host.ctypes.data), "cur_pos3f is not device memory")
    refused(src(prev_p=host.ctypes.data), "prev_pos3f is not device memory")
    refused(src(), "motion3f is not device memory", mo=host.ctypes.data)
    for name, count, per in (("motion3f", N, 12), ("cur_pos3f", nv, 12), ("prev_pos3f", nv, 12)):
        short = C.c_void_p(None)
        assert hip.hipMalloc(C.byref(short), (count * per - 1) // 4096 * 4096) == 0      # whole pages, and too few of them
        try:
            if name == "motion3f":
                refused(src(), "motion3f is smaller than", mo=short.value)
            else:
                refused(src(**{("cur_p" if name == "cur_pos3f" else "prev_p"): short.value}), name + " is smaller than")
        finally:
            hip.hipFree(short)
    hostbuf = art.ArtAovBuffers(); hostbuf.depth = host.ctypes.data
    assert L.art_render_aovs_motion_device(C.byref(p), C.byref(hostbuf), C.byref(src()), motion.data_ptr(), None) != 0
    assert "depth is not device memory" in L.art_last_error().decode()
    # the scene is what it was, and the same arguments, unbroken, are accepted: with planes, with a null ArtAovBuffers, with none wanted
    aov.assert_planes(backend.render_aovs_torch(p, ALL), before, what="after the refusals")
    s = src()
    assert L.art_render_aovs_motion_device(C.byref(p), C.byref(buf), C.byref(s), motion.data_ptr(), None) == 0
    assert L.art_render_aovs_motion_device(C.byref(p), None, C.byref(s), motion.data_ptr(), None) == 0
    assert L.art_render_aovs_motion_device(C.byref(p), C.byref(art.ArtAovBuffers()), C.byref(s), motion.data_ptr(), None) == 0
    assert L.art_render_aovs_motion_device(C.byref(p), C.byref(buf), None, None, None) == 0          # motion3f NULL: the old call, src not read
    torch.cuda.synchronize()
    assert not bool((motion == -7.0).any())
    # an instanced scene refuses vertex arrays and a wrong count
    sd = scenes.instanced_scene(3, 200)
    backend.upload_scene(sd); backend.resize(W, H)
    motion.fill_(-7.0); depth.fill_(-7.0)
    refused(src(), "the scene is instanced")
    refused(src(None, None, 0, mats.data_ptr(), 4), "n_instances 4 differs from the uploaded count 3")
    refused(src(None, None, 0, host.ctypes.data, 3), "prev_m12f is not device memory")
    short = C.c_void_p(None)
    assert hip.hipMalloc(C.byref(short), 4096) == 0
    try:
        big = scenes.instanced_scene(100, 200)                       # 100 matrices are 4800 bytes
        backend.upload_scene(big); backend.resize(W, H)
        refused(src(None, None, 0, short.value, 100), "prev_m12f is smaller than")
    finally:
        hip.hipFree(short)
    backend.synchronize()


def test_refusals_of_the_temporal_motion_plane(art, backend):
    W, H = 41, 25
    L = backend.lib
    N = W * H
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    t = lambda k, dt=torch.float32: torch.zeros(k * N, dtype=dt, device="cuda")
    color, mom, nrm, dep, ids, mo, hin, hout = t(3), t(2), t(3), t(1), t(1, torch.int32), t(3), t(12), t(12)
    host = np.zeros(3 * N, F)
    p = art.ArtTemporalParams()
    p.cur = p.prev = backend.temporal_camera(T.cam(), W, H)
    p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = 2, 16, 1.0, 0.05, 0.9
    args = lambda m: [C.byref(p)] + [x.data_ptr() for x in (color, mom, nrm, dep, ids)] + [m, hin.data_ptr(), hout.data_ptr(), None, None, None, None]
    hout.fill_(-7.0)
    assert L.art_temporal_motion_device(*args(host.ctypes.data)) != 0
    assert "motion3f is not device memory" in L.art_last_error().decode()
    short = C.c_void_p(None)
    assert hip.hipMalloc(C.byref(short), (N - 1) * 12) == 0
    try:
        assert L.art_temporal_motion_device(*args(short.value)) != 0
        assert "motion3f is smaller than" in L.art_last_error().decode()
    finally:
        hip.hipFree(short)
    torch.cuda.synchronize()
    assert bool((hout == -7.0).all())
    assert L.art_temporal_motion_device(*args(mo.data_ptr())) == 0
    torch.cuda.synchronize()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_translating_mesh(art, backend, flat):
    """four frames of the flat scene with the soup translating: refit, a 4-spp pass with accum and moments bound, the feature buffers
    with motion, temporal with motion -- everything on the GPU; the references fed with the GPU's own render outputs give the same bits"""
    W = H = 48
    sd = flat["sd"]
    base = flat["poses"][0]
    p = art.Backend.pass_params(art.PT_MIS, False, 8, 1, seed=5)
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    cam = (np.array(list(sd.desc.cam_pos), F), np.eye(4, dtype=F))
    dirs = aov.camera_dirs(sd.desc, W, H, False)
    h_gpu, h_ref, prev_pos = None, None, base
    try:
        backend.upload_scene(sd)
        backend.bind_accum(accum)
        backend.bind_moments(moments)
        for k in range(4):
            cur_pos = (base + np.array([0.06 * k, 0.0, 0.0], F)).astype(F)
            backend.refit_torch(gpu(cur_pos))
            backend.resize(W, H)
            spp = 0
            for _ in range(4):
                spp = backend.render_pass_device(p, spp)
            aovs = backend.render_aovs_torch_motion(p, ("albedo", "normal", "depth", "prim_index"), cur_pos=gpu(cur_pos), prev_pos=gpu(prev_pos))
            cur = dict(aovs, color=accum, moments=moments)
            out, var, length, h_gpu = backend.temporal_torch(cur, h_gpu, cam, cam if k else None, spp, scale=1.0 / spp, motion=aovs["motion"])
            torch.cuda.synchronize()
            hst = {n: v.cpu().numpy() for n, v in aovs.items()}
            raw = aov.reference(art, backend, sd, W, H, False)[1]
            mo = M.from_hits(raw, dirs, cam[0], idx=flat["idx"], cur=cur_pos, prev=prev_pos).reshape(H, W, 3)
            assert M.differ(hst["motion"], mo) == 0, "frame %d" % k
            r = TM.temporal(accum.cpu().numpy(), moments.cpu().numpy(), spp, cam, cam_prev=cam if k else None, hist=h_ref, normal=hst["normal"],
                            depth=hst["depth"], ids=hst["prim_index"], max_history=art.TEMPORAL_MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL,
                            normal_min=art.TEMPORAL_NORMAL_MIN, scale=1.0 / spp, motion=mo)
            assert spp == 4 and same((h_gpu.cpu().numpy(), out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy()), r), "frame %d" % k
            moving = (np.abs(mo).sum(-1) > 0)
            if k:
                assert moving.sum() > 30
                assert (r[3][moving] > spp).mean() > 0.5, "frame %d: most of the moving mesh found its history" % k
            h_ref, prev_pos = r[0], cur_pos
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)


# ---- quality ------------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_gpu(art, backend):
    """the frames of tests/test_temporal_motion_quality.py rendered on the GPU at equal seeds (the torus moved by refits), their planes
    through the same figures and the same assertions"""
    import temporal_motion_quality as Q
    import test_temporal_motion_quality as TQ
    accum = torch.zeros((Q.H, Q.W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((Q.H, Q.W, 2), dtype=torch.float32, device="cuda")
    frames = []
    try:
        backend.upload_scene(Q.scene(0))
        backend.bind_accum(accum)
        backend.bind_moments(moments)
        for k in range(Q.FRAMES):
            p = art.Backend.pass_params(art.PT_MIS, False, Q.DEPTH, Q.SPP, seed=Q.SEED + k)
            cur, prev = Q.mesh(k), Q.mesh(max(k - 1, 0))
            backend.refit_torch(gpu(cur["pos"]))
            backend.resize(Q.W, Q.H)
            spp = backend.render_pass_device(p, 0)
            aovs = backend.render_aovs_torch_motion(p, ("albedo", "normal", "depth", "prim_type", "prim_index"), cur_pos=gpu(cur["pos"]), prev_pos=gpu(prev["pos"]))
            torch.cuda.synchronize()
            assert spp == Q.SPP
            frames.append((accum.cpu().numpy().copy(), moments.cpu().numpy().copy(), {n: v.cpu().numpy() for n, v in aovs.items()}))
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)
    TQ.check(Q.figures(frames, Q.reference(), art.TEMPORAL_MAX_HISTORY, art.TEMPORAL_DEPTH_TOL, art.TEMPORAL_NORMAL_MIN), Q.record())
