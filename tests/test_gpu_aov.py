"""First-hit feature buffers (art_render_aovs_device through Backend.render_aovs_torch): albedo, normal, depth, alpha and the ids of every
pixel, bit for bit against a reference put together in the test from parts that are held to the oracle elsewhere:
  directions   tests/ada_transcription.eye_ray_direction + the camera matrix in numpy float32 (the recipe of tests/test_sampling_kat.py)
  hits         Backend.trace_rays on those rays
  albedo       a numpy table written from the comment in include/art_hip.h
  sums         (((v0 + v1) + v2) + v3) * 0.25 in numpy float32
No tolerance anywhere: float planes are compared as uint32."""
import ctypes as C

import numpy as np
import pytest

import ada_transcription as ada
import hostsim

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
ALL = ("albedo", "normal", "depth", "alpha", "prim_type", "prim_index", "mat")
SEED = 0xADA5EED0 + 64           # scenes.instanced_scene's default placement; SEED + 1: another one


# ------------------------------------------------------------------------------------------------ the reference
def camera_dirs(desc, W, H, aa):
    """[K, H*W, 3]: ray s of pixel y*W + x (ray_tracer.adb:61-97 + the camera matrix, integrators.adb:37-58)"""
    x = np.tile(np.arange(W), H).astype(F); y = np.repeat(np.arange(H), W).astype(F)
    third = (F(1.0 / 3.0), F(2.0 / 3.0))
    cm = [F(v) for v in desc.cam_matrix]
    out = []
    for s in range(4 if aa else 1):
        ox, oy = (third[(s >> 1) & 1], third[s & 1]) if aa else (F(0.5), F(0.5))       # Generate4RayDirections order
        d0 = ada.eye_ray_direction(x, y, ox, oy, W, H)
        d = ada.normalize(tuple(cm[4 * r] * d0[0] + cm[4 * r + 1] * d0[1] + cm[4 * r + 2] * d0[2] + cm[4 * r + 3] for r in range(3)))
        out.append(np.stack([np.broadcast_to(c, x.shape) for c in d], -1).astype(F))
    return np.stack(out)


def albedo_table(art, desc):
    """include/art_hip.h: LAMBERT, MIRROR, PHONG p[0..2]; GLASS and LIGHT (1, 1, 1); NULL (0, 0, 0)"""
    t = np.zeros((desc.n_materials, 3), F); types = np.zeros(desc.n_materials, np.int32)
    for i in range(desc.n_materials):
        m = desc.materials[i]
        types[i] = m.type
        if m.type in (art.MAT_LAMBERT, art.MAT_MIRROR, art.MAT_PHONG):
            t[i] = [m.p[0], m.p[1], m.p[2]]
        elif m.type in (art.MAT_GLASS, art.MAT_LIGHT):
            t[i] = 1.0
    return t, types


def host_raw(hits):
    return np.frombuffer(C.string_at(C.addressof(hits), C.sizeof(hits)), np.int32).reshape(-1, 11)


def mean4(v):
    """v[K, ...] float32 -> the pixel value in the header's association"""
    return v[0] if v.shape[0] == 1 else ((((v[0] + v[1]) + v[2]) + v[3]) * F(0.25)).astype(F)


def reference(art, backend, sd, W, H, aa, bg=(0.0, 0.0, 0.0)):
    """the seven planes of the uploaded scene sd, and the ArtHit words [K, H*W, 11] they were made from"""
    desc = sd.desc
    d = camera_dirs(desc, W, H, aa)
    K, N = d.shape[0], W * H
    o = np.tile(np.array(list(desc.cam_pos), F), (K * N, 1))
    raw = host_raw(backend.trace_rays(o, np.ascontiguousarray(d.reshape(-1, 3)))).reshape(K, N, 11)
    f = raw.view(F)
    hit = raw[:, :, 1] == 1
    table, _ = albedo_table(art, desc)
    mat = raw[:, :, 5]
    alb = np.where(hit[:, :, None], table[np.where(hit, mat, 0)], np.array(bg, F)).astype(F)
    nrm = np.where(hit[:, :, None], f[:, :, 6:9], F(0.0)).astype(F)
    dep = np.where(hit, f[:, :, 0], F(0.0)).astype(F)
    cov = hit.astype(F)
    ref = dict(albedo=mean4(alb).reshape(H, W, 3), normal=mean4(nrm).reshape(H, W, 3), depth=mean4(dep).reshape(H, W), alpha=mean4(cov).reshape(H, W),
               prim_type=raw[0, :, 2].reshape(H, W), prim_index=raw[0, :, 3].reshape(H, W), mat=raw[0, :, 5].reshape(H, W))
    return ref, raw


def words(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int32, copy=False).view(np.uint32)


def assert_planes(got, want, names=ALL, what=""):
    for name in names:
        g, w = words(got[name]), words(want[name])
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, "%s %s: %d of %d words differ, first at %s: got %#x want %#x" % (what, name, bad.shape[0], w.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


def planes_differ(a, b, name="depth"):
    return not np.array_equal(words(a[name]), words(b[name]))


def aovs(art, backend, aa, bg=(0.0, 0.0, 0.0), want=ALL):
    # render_type, max_depth, vthreads, seed and layout are ignored by the call: values a render pass would refuse prove it
    p = art.Backend.pass_params(art.RT_DEBUG, aa, 0, 0, seed=12345, background=bg, layout=art.LAYOUT_ADA_XY)
    out = backend.render_aovs_torch(p, want)
    assert set(out) == set(want)
    for name in want:
        t = out[name]
        assert t.is_cuda and tuple(t.shape) == ((backend.height, backend.width, 3) if name in ("albedo", "normal") else (backend.height, backend.width))
        assert t.dtype == (torch.float32 if name in ("albedo", "normal", "depth", "alpha") else torch.int32)
    return out


# ------------------------------------------------------------------------------------------------ 1, 2: the reference's scene, slicing
@pytest.fixture(scope="module")
def ref_scene():
    from ada_ray_tracer_amd import scenes
    return scenes.reference_scene()          # spheres, Cornell box, the sphere light, the REFERENCE_BF pyramid


@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("frame", [(1, 1), (67, 5), (257, 3), (61, 47)])
def test_reference_scene(art, backend, ref_scene, frame, aa):
    W, H = frame
    backend.upload_scene(ref_scene); backend.resize(W, H)
    want, raw = reference(art, backend, ref_scene, W, H, aa)
    assert_planes(aovs(art, backend, aa), want)
    if H > 5:                                           # (the flat frames see a strip of the walls and the open front of the box)
        assert set(np.unique(want["prim_type"]).tolist()) == {-1, 0, 1, 2}       # misses, walls, spheres, the pyramid


def test_slices_with_boundaries_inside_rows(art, backend, ref_scene):
    W, H = 67, 5
    backend.upload_scene(ref_scene); backend.resize(W, H)
    whole = aovs(art, backend, True)
    backend.set_option("query_slice", 100)          # 25 pixels of 4 rays per slice: 14 slices, the boundaries inside rows
    try:
        sliced = aovs(art, backend, True)
        sliced_1 = aovs(art, backend, False)        # 100 pixels of 1 ray
    finally:
        backend.set_option("query_slice", 1 << 24)
    assert_planes(sliced, whole, what="sliced")
    want, _ = reference(art, backend, ref_scene, W, H, True)
    assert_planes(sliced, want, what="sliced")
    assert_planes(sliced_1, reference(art, backend, ref_scene, W, H, False)[0], what="sliced, AA off")


# ------------------------------------------------------------------------------------------------ 3: tilted camera, misses, background
def open_scene(art):
    """three spheres and the light in empty space (no Cornell box: camera rays miss) behind tests/test_gpu_parity.py's tilted, translated camera"""
    from ada_ray_tracer_amd import scenes
    c, s = F(np.cos(0.2)), F(np.sin(0.2))
    m = np.array([[c, 0, s, 0.05], [0, 1, 0, -0.02], [-s, 0, c, 0.01], [0, 0, 0, 1]], F)
    spheres = [((-1.5, 1.0, 1.5), 1.0, 8), ((1.4, 1.0, 3.0), 1.0, 0), ((0.3, 3.0, 2.0), 0.7, 2), ((0.0, 4.5, 1.0), 0.5, 4)]
    light = dict(shape=art.LIGHT_SPHERE, mat=4, center=(0.0, 4.5, 1.0), radius=0.5, intensity=(10.0, 10.0, 10.0), surfaceArea=float(F(4.0) * F(np.pi) * F(0.25)))
    return art.SceneDesc(spheres=spheres, lights=[light], materials=scenes.cornell_materials(), meshes=[], cornell=None, cam_pos=(0.4, 2.4, 11.0), cam_matrix=m)


@pytest.mark.parametrize("aa", [True, False])
def test_tilted_camera_misses_and_background(art, backend, aa):
    W, H, bg = 72, 56, (0.1, 0.2, 0.3)
    sd = open_scene(art)
    backend.upload_scene(sd); backend.resize(W, H)
    want, _ = reference(art, backend, sd, W, H, aa, bg)
    a = want["alpha"]
    assert (a == 0).any() and (a == 1).any()
    if aa:
        assert ((a > 0) & (a < 1)).any()                    # silhouettes: some of the pixel's four rays hit
    assert np.array_equal(words(want["albedo"][a == 0]), words(np.broadcast_to(np.array(bg, F), want["albedo"][a == 0].shape)))
    assert_planes(aovs(art, backend, aa, bg), want)
    assert planes_differ(aovs(art, backend, aa, (0.0, 0.0, 0.0)), want, "albedo")      # the background is read from the call


# ------------------------------------------------------------------------------------------------ 4: every primitive and material type
def every_type_scene(art, n_tris=900):
    """Cornell walls (planes), a Phong sphere, a rect light (quad) and a CLOSEST soup whose material ids cycle Lambert, mirror, glass,
    Phong, null and the light"""
    from ada_ray_tracer_amd import scenes
    mesh = scenes.random_triangles(n_tris, 0xADA5EED0 + 31)
    mesh["matid"] = np.array([(1, 5, 0, 8, 6, 4)[i % 6] for i in range(n_tris)], np.int32)
    lights = [scenes.rect_light(0.0, 4, half_x=1.0, half_z=1.0)]
    return art.SceneDesc(spheres=[((-1.5, 1.0, 1.5), 1.0, 8)], lights=lights, materials=scenes.cornell_materials(), meshes=[mesh],
                         cornell=scenes.CORNELL_BOX, cam_pos=scenes.REFERENCE_CAMERA)


@pytest.mark.parametrize("aa", [True, False])
def test_every_primitive_and_material_type(art, backend, aa):
    W, H = 96, 80
    sd = every_type_scene(art)
    backend.upload_scene(sd); backend.resize(W, H)
    want, raw = reference(art, backend, sd, W, H, aa)
    hit = raw[:, :, 1] == 1
    _, types = albedo_table(art, sd.desc)
    assert set(np.unique(raw[:, :, 2][hit]).tolist()) == {0, 1, 2, 3}
    assert set(np.unique(types[raw[:, :, 5][hit]]).tolist()) == {art.MAT_NULL, art.MAT_LIGHT, art.MAT_LAMBERT, art.MAT_MIRROR, art.MAT_GLASS, art.MAT_PHONG}
    assert_planes(aovs(art, backend, aa), want)


# ------------------------------------------------------------------------------------------------ 5: an instanced scene
def small_instanced(k=0):
    from ada_ray_tracer_amd import scenes
    return scenes.instanced_scene(8, 300, seed=SEED + k)


def test_instanced_scene_equals_its_flattened_copy(art, backend):
    W, H = 96, 80
    sd = small_instanced()
    flat = hostsim.flattened_copy(art, sd)
    backend.upload_scene(sd); backend.resize(W, H)
    want, raw = reference(art, backend, sd, W, H, True)
    got = aovs(art, backend, True)
    assert_planes(got, want, what="instanced")              # prim_index: instance << shift | triangle, as trace_rays reports it here
    on_mesh = want["prim_type"] == 2
    assert on_mesh.sum() > 100 and len(np.unique(want["prim_index"][on_mesh] >> 9)) >= 3      # (meshes of 2^8 < n <= 2^9 triangles) several instances are seen
    backend.upload_scene(flat); backend.resize(W, H)
    got_flat = aovs(art, backend, True)
    assert_planes(got, got_flat, [n for n in ALL if n != "prim_index"], what="instanced against flattened")
    off = ~on_mesh
    assert np.array_equal(words(got["prim_index"])[off], words(got_flat["prim_index"])[off])
    backend.set_option("trace_kernel", 1)
    try:
        backend.upload_scene(sd); backend.resize(W, H)
        with pytest.raises(art.ArtError, match="trace_kernel"):
            aovs(art, backend, True)
    finally:
        backend.set_option("trace_kernel", 0)


# ------------------------------------------------------------------------------------------------ 6: updates enqueued before the call are seen
def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).cuda()


def test_a_refit_enqueued_before_the_call_is_seen(art, backend):
    from ada_ray_tracer_amd import scenes
    W, H = 96, 80
    sd = scenes.synthetic_scene(2000, 3)
    pos, nrm, idx, _, matid = sd._mesh_arrays[-1]
    moved_pos = (pos.astype(np.float64) + np.array([0.11, -0.07, 0.23])).astype(F)
    moved = art.SceneDesc(meshes=[dict(mode=art.MESH_CLOSEST, pos=moved_pos, nrm=nrm, idx=idx, matid=matid)], **sd._kw)
    backend.upload_scene(moved); backend.resize(W, H)
    want = aovs(art, backend, True)
    backend.upload_scene(sd); backend.resize(W, H)
    before = aovs(art, backend, True)
    backend.refit_torch(gpu(moved_pos), check=False)        # (check=False: no host synchronisation between the two calls)
    got = aovs(art, backend, True)
    assert planes_differ(before, want)
    assert_planes(got, want, what="after a refit")
    backend.synchronize()


def test_a_move_enqueued_before_the_call_is_seen(art, backend):
    W, H = 96, 80
    A, B = small_instanced(0), small_instanced(1)
    mats_b = np.array([list(B.desc.instances[i].m) for i in range(B.desc.n_instances)], F)
    backend.upload_scene(B); backend.resize(W, H)
    want = aovs(art, backend, True)
    backend.upload_scene(A); backend.resize(W, H)
    before = aovs(art, backend, True)
    backend.move_instances_torch(gpu(mats_b), check=False)
    got = aovs(art, backend, True)
    assert planes_differ(before, want)
    assert_planes(got, want, what="after a move")
    backend.synchronize()


# ------------------------------------------------------------------------------------------------ 7: no side effects
def test_a_call_between_two_passes_changes_nothing(art, backend, ref_scene):
    """Accum bits, spp, ArtStats' counts and ArtStageStats' counts after pass + call + pass equal those after pass + pass.  (The GPU times
    in both structures differ from run to run, with or without the call: the launch counts next to them are compared instead.)"""
    W, H = 64, 48
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 2, seed=5)
    backend.upload_scene(ref_scene)

    def two_passes(between):
        backend.resize(W, H)
        _, _, spp = backend.render_pass(p, 0, want_accum=False)
        between()
        accum, _, spp = backend.render_pass(p, spp)
        st, sg = backend.stats(), backend.stage_stats()
        return (words(accum).copy(), spp, (st.rays, st.samples, st.trace_launches, st.lost_paths),
                (sg.shade_launches, sg.batches, list(sg.items_in), list(sg.items_out)), backend.camera_rays_traced())

    plain = two_passes(lambda: None)
    seen = []
    with_call = two_passes(lambda: seen.append(aovs(art, backend, True)))
    assert plain[1] == with_call[1] == 16 and np.array_equal(plain[0], with_call[0])
    assert plain[2:] == with_call[2:]
    assert_planes(seen[0], reference(art, backend, ref_scene, W, H, True)[0])


# ------------------------------------------------------------------------------------------------ 8: subsets and refusals
def test_wanted_subsets_equal_the_full_call(art, backend):
    W, H = 67, 5
    sd = every_type_scene(art)
    backend.upload_scene(sd); backend.resize(W, H)
    for aa in (True, False):
        full = aovs(art, backend, aa)
        for want in (("depth",), ("prim_type", "prim_index", "mat"), ("mat",), ("normal",), ("albedo", "alpha")):
            assert_planes(aovs(art, backend, aa, want=want), full, want, what="subset %s" % (want,))


def test_host_memory_is_refused(art, backend, ref_scene):
    backend.upload_scene(ref_scene); backend.resize(16, 8)
    p = art.Backend.pass_params()
    L = backend.lib
    host = torch.zeros((8, 16), dtype=torch.float32)
    buf = art.ArtAovBuffers(); buf.depth = host.data_ptr()
    assert L.art_render_aovs_device(C.byref(p), C.byref(buf), None) != 0
    assert "depth is not device memory" in L.art_last_error().decode()
    assert L.art_render_aovs_device(C.byref(p), C.byref(art.ArtAovBuffers()), None) != 0
    assert "all seven pointers are null" in L.art_last_error().decode()
    with pytest.raises(ValueError):
        backend.render_aovs_torch(p, want=("nope",))


# ------------------------------------------------------------------------------------------------ 9: a path that shares no code with the queries
def test_ids_agree_with_the_debug_pass(art, backend, ref_scene):
    """art_debug_hit_pass (k_debug) reports prim_index, prim_type and mat_id at pixel centres.  mat_id is the material only where the
    primitive carries its own (walls, triangles); a sphere's material comes from the sphere table, which the debug pass does not
    report, so there the mat plane is held to the scene description through the debug pass's sphere index."""
    W, H = 80, 64
    backend.upload_scene(ref_scene); backend.resize(W, H)
    got = aovs(art, backend, False, want=("prim_type", "prim_index", "mat"))
    _, _, prim, mat_id, ptype = backend.debug_hit_pass(art.Backend.pass_params(art.RT_DEBUG, False, 8, 1))      # row-major: [H, W]
    assert_planes(got, dict(prim_type=ptype, prim_index=prim), ("prim_type", "prim_index"))
    mat = got["mat"].cpu().numpy()
    sphere = ptype == 1
    assert sphere.sum() > 50 and (ptype == 0).sum() > 50 and (ptype == 2).sum() > 10
    assert np.array_equal(mat[~sphere], mat_id[~sphere])
    d = ref_scene.desc
    sphere_mat = np.array([d.spheres[i].mat for i in range(d.n_spheres)], np.int32)
    assert np.array_equal(mat[sphere], sphere_mat[prim[sphere]])
