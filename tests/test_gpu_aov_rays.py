"""Feature buffers along the caller's rays (art_aovs_rays_device through Backend.aovs_rays_torch) and the frame's camera rays
(art_camera_rays_device through Backend.camera_rays_torch), bit for bit:
  camera rays   against test_gpu_aov.camera_dirs (the numpy transcription of the reference's ray generation) and cam_pos
  composition   the camera rays fed back with group = K against render_aovs_torch
  caller rays   against tests/aov_rays_ref.py (numpy, written from the header) fed with trace_rays_torch's ArtHit words
No tolerance anywhere: float planes are compared as uint32."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import aov_rays_ref
from test_gpu_aov import albedo_table, assert_planes, camera_dirs, every_type_scene, words

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
ALL = aov_rays_ref.PLANES
SHARED = tuple(n for n in ALL if n != "position")
SENTINEL_F, SENTINEL_I = -777.25, -77777
DEFAULT_SLICE = 1 << 24


# ------------------------------------------------------------------------------------------------ scenes and rays, made once
_scenes = {}


def scene(art, name):
    if name not in _scenes:
        from ada_ray_tracer_amd import scenes
        _scenes[name] = {"ref": lambda: scenes.reference_scene(),            # spheres, Cornell box, the sphere light, the REFERENCE_BF pyramid
                         "soup": lambda: every_type_scene(art),              # walls, a sphere, a rect light, a 900-triangle CLOSEST soup of every material
                         "inst": lambda: scenes.instanced_scene(8, 300)}[name]()
    return _scenes[name]


def gpu(a, dtype=F):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def random_rays(n, seed):
    """origins spread through the box (so that a sphere's normal depends on the ray's own origin), directions of any length"""
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3)) * np.array([4.6, 4.6, 4.6]) + np.array([-2.3, 0.2, 0.2])).astype(F)
    d = (rng.standard_normal((n, 3)) * 2.0 ** rng.uniform(-2.0, 2.0, (n, 1))).astype(F)
    return o, d


def reference(art, backend, sd, o, d, group, bg, tnear=None, tfar=None, kernel=0):
    """the eight planes of aov_rays_ref from trace_rays_torch's words for the same rays and interval (kernel: what the option trace_kernel holds)"""
    hits = backend.trace_rays_torch(gpu(o), gpu(d), None if tnear is None else gpu(tnear), None if tfar is None else gpu(tfar), kernel)
    table, _ = albedo_table(art, sd.desc)
    return aov_rays_ref.aov_rays_ref(hits.raw.cpu().numpy(), o, d, group, bg, table), hits.raw.cpu().numpy()


def call(backend, o, d, group, bg=(0.0, 0.0, 0.0), tnear=None, tfar=None, want=ALL, out=None):
    got = backend.aovs_rays_torch(gpu(o), gpu(d), group, None if tnear is None else gpu(tnear), None if tfar is None else gpu(tfar), bg, want, out)
    g = o.shape[0] // group
    assert set(got) == set(want)
    for name in want:
        t = got[name]
        assert t.is_cuda and tuple(t.shape) == ((g, 3) if name in ("albedo", "normal", "position") else (g,))
        assert t.dtype == (torch.int32 if name in ("prim_type", "prim_index", "mat") else torch.float32)
    return got


def sentinels(g, device="cuda"):
    return {name: torch.full((g, 3) if name in ("albedo", "normal", "position") else (g,), SENTINEL_I if name in ("prim_type", "prim_index", "mat") else SENTINEL_F,
                             dtype=torch.int32 if name in ("prim_type", "prim_index", "mat") else torch.float32, device=device) for name in ALL}


def untouched(planes, names=ALL):
    return all(bool((planes[n] == (SENTINEL_I if planes[n].dtype == torch.int32 else SENTINEL_F)).all()) for n in names)


# ------------------------------------------------------------------------------------------------ 1: the camera rays
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("frame", [(1, 1), (67, 5), (257, 3)])
def test_camera_rays_are_the_reference_ray_generation(art, backend, frame, aa):
    W, H = frame
    sd = scene(art, "ref")
    backend.upload_scene(sd); backend.resize(W, H)
    K = 4 if aa else 1
    p = art.Backend.pass_params(art.RT_DEBUG, aa, 0, 0, seed=99, background=(0.3, 0.2, 0.1), layout=art.LAYOUT_ADA_XY)      # only aa_on is read
    o, d = backend.camera_rays_torch(p)
    assert o.is_cuda and d.is_cuda and tuple(o.shape) == tuple(d.shape) == (H * W * K, 3) and o.dtype == d.dtype == torch.float32
    want_d = np.ascontiguousarray(camera_dirs(sd.desc, W, H, aa).transpose(1, 0, 2)).reshape(-1, 3)      # [K, N, 3] -> ray s of pixel q at q * K + s
    want_o = np.tile(np.array(list(sd.desc.cam_pos), F), (H * W * K, 1))
    assert np.array_equal(words(o), words(want_o))
    bad = np.argwhere(words(d) != words(want_d))
    assert bad.shape[0] == 0, "%d direction words differ, first at %s" % (bad.shape[0], tuple(bad[0]))


# ------------------------------------------------------------------------------------------------ 2: composition
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("name", ["ref", "soup", "inst"])
def test_camera_rays_fed_back_give_the_frames_planes(art, backend, name, aa):
    W, H, bg = 61, 47, (0.1, 0.2, 0.3)
    backend.upload_scene(scene(art, name)); backend.resize(W, H)
    p = art.Backend.pass_params(art.PT_MIS, aa, 8, 1, background=bg)
    want = backend.render_aovs_torch(p)
    o, d = backend.camera_rays_torch(p)
    got = backend.aovs_rays_torch(o, d, group=4 if aa else 1, background=bg)
    assert (want["alpha"] == 0).any() or name != "ref"                        # (the reference scene's open front: the background is in play)
    assert_planes({n: got[n].reshape(want[n].shape) for n in SHARED}, want, SHARED, what="%s aa=%s" % (name, aa))
    pos = got["position"].cpu().numpy(); hit = want["alpha"].cpu().numpy().reshape(-1) == 1
    assert hit.sum() > 100 and np.isfinite(pos).all() and (np.abs(pos[hit]) <= 12.6).all()


# ------------------------------------------------------------------------------------------------ 3: caller rays against the reference
@pytest.mark.parametrize("name", ["ref", "soup", "inst"])
def test_caller_rays_equal_the_reference(art, backend, name):
    sd = scene(art, name)
    backend.upload_scene(sd)
    bg = (0.25, 0.5, 0.75)
    seen_types, spheres_from_two_sides = set(), 0
    for group in (1, 3, 4, 16):
        for groups in (1, 255, 256, 257, 1000):            # the LDS staging tail, a block edge, several blocks
            o, d = random_rays(group * groups, 1000 * group + groups)
            want, raw = reference(art, backend, sd, o, d, group, bg)
            got = call(backend, o, d, group, bg)
            assert_planes(got, want, ALL, what="%s group %d x %d" % (name, group, groups))
            seen_types |= set(np.unique(raw[:, 2]).tolist())
            spheres_from_two_sides += int((raw[:, 2] == 1).sum())
    assert {-1, 0, 2} <= seen_types and (name == "inst" or 1 in seen_types) and (name != "soup" or 3 in seen_types)
    assert name == "inst" or spheres_from_two_sides > 100


# ------------------------------------------------------------------------------------------------ 4: bounds
@pytest.mark.parametrize("name", ["ref", "soup", "inst"])
def test_bounds_follow_the_queries_interval_rule(art, backend, name):
    sd = scene(art, name)
    backend.upload_scene(sd)
    group, groups, bg = 4, 700, (0.9, 0.1, 0.4)
    n = group * groups
    o, d = random_rays(n, 4242)
    free, raw = reference(art, backend, sd, o, d, group, bg)
    t = raw.view(F)[:, 0]; hit = raw[:, 1] == 1
    rng = np.random.default_rng(7)
    kind = rng.integers(0, 6, n)
    th = np.where(hit, t, F(1.0))                          # (a miss's t is the bound, Float'Last: its intervals are drawn, not derived)
    tnear = np.where(kind == 0, -1.0, np.where(kind == 1, th * 0.5, np.where(kind == 2, th * 1.5, rng.random(n) * 2.0))).astype(F)      # negative: no shift | before the hit | past it
    tfar = np.where(kind == 3, th * 0.5, np.where(kind == 4, tnear, np.where(kind == 5, tnear * 0.5, 3.0e38))).astype(F)              # cuts the hit off | empty | empty
    want, raw_b = reference(art, backend, sd, o, d, group, bg, tnear, tfar)
    hit_b = raw_b[:, 1] == 1
    assert (hit & ~hit_b).sum() > 100 and hit_b.sum() > 100 and (hit_b & (raw_b.view(F)[:, 0] != t)).sum() > 50      # hits cut off, hits kept, hits further on
    got = call(backend, o, d, group, bg, tnear, tfar)
    assert_planes(got, want, ALL, what=name + " bounded")
    only_near = call(backend, o, d, group, bg, tnear=tnear)
    assert_planes(only_near, reference(art, backend, sd, o, d, group, bg, tnear)[0], ALL, what=name + " tnear alone")
    only_far = call(backend, o, d, group, bg, tfar=tfar)
    assert_planes(only_far, reference(art, backend, sd, o, d, group, bg, None, tfar)[0], ALL, what=name + " tfar alone")
    assert not np.array_equal(words(got["depth"]), words(free["depth"]))


# ------------------------------------------------------------------------------------------------ 5: slicing
def test_slices_of_whole_groups_give_the_same_words(art, backend):
    sd = scene(art, "soup")
    backend.upload_scene(sd)
    bg = (0.2, 0.3, 0.4)
    o, d = random_rays(16 * 75, 31)
    rng = np.random.default_rng(32)
    tnear = (rng.random(o.shape[0]) * 0.5).astype(F); tfar = (rng.random(o.shape[0]) * 8.0).astype(F)
    whole = {g: call(backend, o, d, g, bg, tnear, tfar) for g in (16, 3, 1)}
    assert_planes(whole[16], reference(art, backend, sd, o, d, 16, bg, tnear, tfar)[0], ALL, what="default slice")
    unbounded = call(backend, o[:48], d[:48], 3, bg)
    try:
        backend.set_option("query_slice", 64)           # 4 groups of 16, 21 of 3, 64 of 1
        for g in (16, 3, 1):
            assert_planes(call(backend, o, d, g, bg, tnear, tfar), whole[g], ALL, what="slices of 64 rays, group %d" % g)
        backend.set_option("query_slice", 7)            # smaller than a group of 16: one group per slice
        assert_planes(call(backend, o, d, 16, bg, tnear, tfar), whole[16], ALL, what="slices of 7 rays, group 16")
        assert_planes(call(backend, o[:48], d[:48], 3, bg), unbounded, ALL, what="slices of 7 rays, group 3, no bounds")      # two groups per slice
    finally:
        backend.set_option("query_slice", DEFAULT_SLICE)
    assert_planes(call(backend, o, d, 16, bg, tnear, tfar), whole[16], ALL, what="default slice again")


# ------------------------------------------------------------------------------------------------ 6: plane subsets
def test_each_plane_alone_equals_the_full_call_and_leaves_the_others_alone(art, backend):
    backend.upload_scene(scene(art, "soup"))
    group, groups, bg = 3, 300, (0.6, 0.5, 0.4)
    o, d = random_rays(group * groups, 66)
    full = call(backend, o, d, group, bg)
    for name in ALL:
        planes = sentinels(groups)
        got = call(backend, o, d, group, bg, want=(name,), out={name: planes[name]})
        assert got[name] is planes[name]
        assert_planes(got, full, (name,), what="%s alone" % name)
    # the C entry with one pointer set: the seven other tensors of the struct's layout stay as they were
    L = backend.lib
    og, dg = gpu(o), gpu(d)
    for name in ALL:
        planes = sentinels(groups)
        buf = art.aov_rays.ArtAovRayBuffers()
        setattr(buf, art.aov_rays.RAY_PLANES[name][0], planes[name].data_ptr())
        p = art.aov_rays.ArtAovRaysParams(group, (C.c_float * 3)(*bg))
        assert L.art_aovs_rays_device(C.byref(p), og.data_ptr(), dg.data_ptr(), None, None, group * groups, C.byref(buf), None) == 0, L.art_last_error().decode()
        assert_planes(planes, full, (name,), what="%s alone, C entry" % name)
        assert untouched(planes, [n for n in ALL if n != name])
    for subset in (("albedo", "alpha"), ("prim_type", "prim_index", "mat"), ("position", "depth"), ("normal", "mat")):
        assert_planes(call(backend, o, d, group, bg, want=subset), full, subset, what="subset %s" % (subset,))


# ------------------------------------------------------------------------------------------------ 7: stream order, no side effects
def test_a_call_on_a_side_stream_sees_a_refit_of_the_librarys_stream(art, backend):
    from ada_ray_tracer_amd import scenes
    sd = scenes.synthetic_scene(2000, 3)
    pos, nrm, idx, _, matid = sd._mesh_arrays[-1]
    moved_pos = (pos.astype(np.float64) + np.array([0.11, -0.07, 0.23])).astype(F)
    moved = art.SceneDesc(meshes=[dict(mode=art.MESH_CLOSEST, pos=moved_pos, nrm=nrm, idx=idx, matid=matid)], **sd._kw)
    group, bg = 4, (0.0, 0.1, 0.2)
    o, d = random_rays(group * 3000, 77)
    og, dg, new_pos = gpu(o), gpu(d), gpu(moved_pos)
    backend.upload_scene(moved)
    want = backend.aovs_rays_torch(og, dg, group, background=bg)
    backend.upload_scene(sd)
    before = backend.aovs_rays_torch(og, dg, group, background=bg)
    torch.cuda.synchronize()                               # (the vertices are there before the library's stream reads them)
    assert backend.lib.art_refit_device(new_pos.data_ptr(), None, moved_pos.shape[0], None) == 0, backend.lib.art_last_error().decode()      # NULL: the library's stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = backend.aovs_rays_torch(og, dg, group, background=bg)
    side.synchronize()
    assert not np.array_equal(words(before["depth"]), words(want["depth"]))
    assert_planes(got, want, ALL, what="after a refit")
    backend.synchronize()


def test_calls_between_two_passes_change_nothing(art, backend):
    """Accum bits, spp, ArtStats' counts and ArtStageStats' counts after pass + calls + pass equal those after pass + pass."""
    W, H = 64, 48
    sd = scene(art, "ref")
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 2, seed=5)
    backend.upload_scene(sd)
    o, d = random_rays(4 * 500, 88)

    def two_passes(between):
        backend.resize(W, H)
        _, _, spp = backend.render_pass(p, 0, want_accum=False)
        between()
        accum, _, spp = backend.render_pass(p, spp)
        st, sg = backend.stats(), backend.stage_stats()
        return (words(accum).copy(), spp, (st.rays, st.samples, st.trace_launches, st.lost_paths),
                (sg.shade_launches, sg.batches, list(sg.items_in), list(sg.items_out)), backend.camera_rays_traced())

    def calls():
        co, cd = backend.camera_rays_torch(p)
        seen.append(backend.aovs_rays_torch(co, cd, 4))
        seen.append(call(backend, o, d, 4))

    plain = two_passes(lambda: None)
    seen = []
    with_calls = two_passes(calls)
    assert plain[1] == with_calls[1] == 16 and np.array_equal(plain[0], with_calls[0])
    assert plain[2:] == with_calls[2:]
    assert_planes(seen[1], reference(art, backend, sd, o, d, 4, (0.0, 0.0, 0.0))[0], ALL)
    assert_planes({n: seen[0][n].reshape(H, W, -1).squeeze(-1) if seen[0][n].dim() == 1 else seen[0][n].reshape(H, W, 3) for n in SHARED},
                  backend.render_aovs_torch(p), SHARED)


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_every_refusal_leaves_the_planes_alone(art, backend):
    L = backend.lib
    P, B = art.aov_rays.ArtAovRaysParams, art.aov_rays.ArtAovRayBuffers
    backend.upload_scene(scene(art, "soup"))
    group, groups = 4, 64
    n = group * groups
    o, d = random_rays(n, 99)
    og, dg = gpu(o), gpu(d)
    tn, tf = torch.zeros(n, device="cuda"), torch.full((n,), 9.0, device="cuda")
    planes = sentinels(groups)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p(None)
    assert hip.hipMalloc(C.byref(short), 4 * groups - 4) == 0      # one float short of a scalar plane, far short of the rays

    def buffers(**other):
        b = B()
        for name in ALL:
            setattr(b, art.aov_rays.RAY_PLANES[name][0], other.get(name, planes[name].data_ptr()))
        return b

    def refused(text, p=P(group), rays=n, o_=og.data_ptr(), d_=dg.data_ptr(), tn_=tn.data_ptr(), tf_=tf.data_ptr(), out=None, null_out=False):
        out = buffers() if out is None else out
        rc = L.art_aovs_rays_device(C.byref(p) if p is not None else None, o_, d_, tn_, tf_, rays, None if null_out else C.byref(out), None)
        assert rc != 0 and text in L.art_last_error().decode(), (text, rc, L.art_last_error().decode())
        torch.cuda.synchronize()
        assert untouched(planes), text
    try:
        refused("null ArtAovRaysParams", p=None)
        refused("null ArtAovRayBuffers", null_out=True)
        refused("all eight pointers are null", out=B())
        for k in (0, 17, -1):
            refused("group must be 1..16", p=P(k))
        refused("n_rays must be 0 .. 2^31 - 1", rays=-4)
        refused("n_rays must be 0 .. 2^31 - 1", rays=1 << 31)
        refused("is not a multiple of group 4", rays=n - 1)
        refused("null origins3f or dirs3f", o_=None)
        refused("null origins3f or dirs3f", d_=None)
        host = np.zeros(3 * n, F)
        refused("origins3f is not device memory", o_=host.ctypes.data)
        refused("dirs3f is not device memory", d_=host.ctypes.data)
        refused("tnear is not device memory", tn_=host.ctypes.data)
        refused("tfar is not device memory", tf_=host.ctypes.data)
        for name in ALL:
            field = art.aov_rays.RAY_PLANES[name][0]
            refused(field + " is not device memory", out=buffers(**{name: host.ctypes.data}))
            refused(field + " is smaller than", out=buffers(**{name: short.value}))
        refused("origins3f is smaller than", o_=short.value)
        refused("dirs3f is smaller than", d_=short.value)
        refused("tnear is smaller than", tn_=short.value)
        refused("tfar is smaller than", tf_=short.value)
        # n_rays == 0 succeeds and launches nothing
        assert L.art_aovs_rays_device(C.byref(P(group)), None, None, None, None, 0, C.byref(buffers()), None) == 0
        torch.cuda.synchronize()
        assert untouched(planes)
        # the camera rays: a host array, an array too small
        backend.resize(8, 8)
        pp = art.Backend.pass_params(aa_on=True)
        good = torch.full((8 * 8 * 4, 3), SENTINEL_F, device="cuda")
        for args, text in (((host.ctypes.data, good.data_ptr()), "origins3f is not device memory"), ((good.data_ptr(), host.ctypes.data), "dirs3f is not device memory"),
                           ((short.value, good.data_ptr()), "origins3f is smaller than"), ((good.data_ptr(), short.value), "dirs3f is smaller than")):
            assert L.art_camera_rays_device(C.byref(pp), args[0], args[1], None) != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())
        torch.cuda.synchronize()
        assert bool((good == SENTINEL_F).all())
        # the Python layer: an unknown plane, before any call
        with pytest.raises(ValueError, match="unknown plane"):
            backend.aovs_rays_torch(og, dg, want=("nope",))
        # an instanced scene with the one-ray-per-lane schedule
        backend.upload_scene(scene(art, "inst"))
        backend.set_option("trace_kernel", 1)
        try:
            refused("an instanced scene is traced through the record schedule only")
        finally:
            backend.set_option("trace_kernel", 0)
        # a flat scene with that schedule goes through: the words of the queries' one-ray-per-lane kernel
        backend.upload_scene(scene(art, "soup"))
        want = reference(art, backend, scene(art, "soup"), o, d, group, (0.0, 0.0, 0.0), kernel=art.TRACE_SIMPLE)[0]
        backend.set_option("trace_kernel", 1)
        try:
            assert_planes(call(backend, o, d, group), want, ALL, what="trace_kernel 1")
        finally:
            backend.set_option("trace_kernel", 0)
    finally:
        hip.hipFree(short)


CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import torch
import __graft_entry__ as ge
art = ge.load_package()
from ada_ray_tracer_amd import scenes
import test_gpu_aov_rays as T
be = art.Backend(0)
L = be.lib
P, B = art.aov_rays.ArtAovRaysParams, art.aov_rays.ArtAovRayBuffers
o, d = T.random_rays(64, 5)
og, dg = T.gpu(o), T.gpu(d)
planes = T.sentinels(16)
buf = B()
for name in T.ALL:
    setattr(buf, art.aov_rays.RAY_PLANES[name][0], planes[name].data_ptr())
rays = torch.full((4 * 8 * 8, 3), T.SENTINEL_F, device="cuda")
pp = art.Backend.pass_params(aa_on=True)

def aovs():
    rc = L.art_aovs_rays_device(C.byref(P(4)), og.data_ptr(), dg.data_ptr(), None, None, 64, C.byref(buf), None)
    torch.cuda.synchronize()
    return "%d %s %s" % (rc, T.untouched(planes), L.art_last_error().decode() if rc else "")

def camera():
    rc = L.art_camera_rays_device(C.byref(pp), rays.data_ptr(), rays.data_ptr(), None)
    torch.cuda.synchronize()
    return "%d %s %s" % (rc, bool((rays == T.SENTINEL_F).all()), L.art_last_error().decode() if rc else "")
print(aovs())                                  # no scene
print(camera())                                # no scene
verts = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0); tri = (C.c_int * 3)(0, 1, 2)
L.gcore_init_and_clear()
L.gcore_instance_meshes(L.gcore_add_mesh_3f(verts, 3, tri, 3), (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1), 1)
L.gcore_commit_scene()
print(camera())                                # a scene without a camera
L.gcore_destroy()
sd = scenes.reference_scene()
be.upload_scene(sd)
print(camera())                                # no viewport
print(aovs())                                  # ... which the caller's rays do not need
want, _ = T.reference(art, be, sd, o, d, 4, (0.0, 0.0, 0.0))
print(all(np.array_equal(T.words(planes[n]), T.words(want[n])) for n in T.ALL))
be.shutdown()
be = art.Backend(devices=[0, 0])
be.upload_scene(sd); be.resize(8, 8)
planes = T.sentinels(16)
for name in T.ALL:
    setattr(buf, art.aov_rays.RAY_PLANES[name][0], planes[name].data_ptr())
print(aovs())                                  # two contexts
be.shutdown()
"""


def test_refusals_without_scene_or_frame_and_with_two_contexts(art):
    """a process of its own: the session's backend has a scene, a frame and one context"""
    r = subprocess.run([sys.executable, "-c", CHILD, art.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.strip().split("\n")
    assert out[0].startswith("1 True") and "art_aovs_rays_device: no scene uploaded" in out[0]
    assert out[1].startswith("1 True") and "art_camera_rays_device: no scene uploaded" in out[1]
    assert out[2].startswith("1 True") and "gcore_commit_scene, which has no camera" in out[2]
    assert out[3].startswith("1 True") and "art_camera_rays_device: no viewport" in out[3]
    assert out[4].startswith("0 False") and out[5] == "True"
    assert out[6].startswith("1 True") and "art_aovs_rays_device: not available after art_init_devices" in out[6]
