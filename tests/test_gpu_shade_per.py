"""The shade stage's items per thread, pinned: option shade_per = 2 and = 4 (k_shade_compact<2, *> and <4, *>), set BEFORE the render, so
which instantiation a case runs never depends on a measurement.  Left to itself (shade_per = 0) the library runs 4 items per thread in
the first two batches after an upload, a resize or a batch_paths change, 2 in the third batch of equal size, and then whichever the HIP
events measured faster -- so a suite of one-batch renders only ever runs 4.

Every case is rendered once per value and held to the CPU oracle bit for bit: accum as uint32 words, ArtStats::rays equal to the
oracle's count, lost_paths == 0; the LDR frame equals the oracle's resolve and the frame rendered with the other value.

The stage's chunk is 256 * PER items (512 against 1024), so the frames put the path count on both sides of both:
1x1 (4 paths), 16x8 (512: exactly one chunk at PER 2), 23x11 (1012: a partial chunk at PER 4, a full and a partial one at PER 2),
23x11 without AA (253: below one 256-item round), 33x16 (2112: two full chunks + 64 at PER 4)."""
import numpy as np
import pytest

import conv
import hostsim
import orc

pytestmark = pytest.mark.gpu

PERS = (2, 4)
SEED = 11
DEFAULT_BATCH_PATHS = 128 << 20
# name -> (width, height, anti-aliasing)
FRAMES = {"1x1": (1, 1, True), "16x8": (16, 8, True), "23x11": (23, 11, True), "23x11-noaa": (23, 11, False), "33x16": (33, 16, True), "32x16": (32, 16, True),
          "32x24": (32, 24, True)}
INTEGRATORS = ("PT_MIS", "PT_SHADOW", "PT_STUPID")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lds_overflow_scene(art):
    """the scene of test_gpu_parity.test_more_spheres_and_lights_than_the_stages_keep_in_lds: 70 spheres and 10 sphere lights (more than
    the 64 / 8 the shade stage keeps in LDS: tables_in_lds == false) + a BVH mesh"""
    from ada_ray_tracer_amd import scenes
    rng = np.random.default_rng(5)
    mats = scenes.cornell_materials()
    lights, spheres = [], []
    for k in range(10):
        mats.append(dict(type=art.MAT_LIGHT, light=k)) if k else mats.__setitem__(4, dict(type=art.MAT_LIGHT, light=0))
        m = 4 if k == 0 else len(mats) - 1
        l = scenes.sphere_light(-2.0 + 0.44 * k, m, cy=4.4, cz=1.0 + 0.3 * k, radius=0.12)
        lights.append(l); spheres.append((l["center"], l["radius"], m))
    for k in range(60):
        p = (float(-2.1 + 4.2 * rng.random()), float(0.3 + 3.2 * rng.random()), float(0.4 + 4.0 * rng.random()))
        spheres.append((p, 0.12, (0, 1, 2, 3, 8)[k % 5]))
    mesh = scenes.random_triangles(1500, 0xADA5EED0 + 33)
    return art.SceneDesc(spheres=spheres, lights=lights, materials=mats, meshes=[mesh], cornell=scenes.CORNELL_BOX, cam_pos=scenes.REFERENCE_CAMERA)


_scenes = {}


def scene(art, name):
    """(what the backend uploads, what the oracle renders, the SceneDesc the oracle's scene was made from or None), built once per name"""
    if name not in _scenes:
        from ada_ray_tracer_amd import scenes
        if name == "cornell":                                  # no BVH: the stages' non-staged record path
            cs = orc.CornellScene()
            _scenes[name] = (scenes.reference_scene(), cs, None)
        else:
            sd = {"mixed": lambda: scenes.mixed_scene(1500, 5), "mirror": scenes.mirror_scene,
                  "synthetic": lambda: scenes.synthetic_scene(2000, 3), "rect": lambda: scenes.synthetic_scene(2000, 3, rect_lights=True),
                  "lds": lambda: _lds_overflow_scene(art), "instanced": lambda: scenes.instanced_scene(12, 300)}[name]()
            flat = hostsim.flattened_copy(art, sd) if name == "instanced" else sd      # the oracle renders the explicit world-space mesh
            _scenes[name] = (sd, conv.OracleScene(flat), flat)
    return _scenes[name]


_oracle = {}


def oracle_frame(art, name, rt, frame, depth, vthreads=1):
    """The oracle's picture of one (scene, integrator, frame, depth, samples): computed once, shared by both shade_per values and never
    changed.  (accum bits, LDR frame, spp, rays)"""
    key = (name, rt, frame, depth, vthreads)
    if key not in _oracle:
        w, h, aa = FRAMES[frame]
        ref, spp, cnt = orc.render(scene(art, name)[1].scene, orc.make_params(w, h, getattr(orc, rt), aa, depth, vthreads, seed=SEED))
        acc = bits(ref).copy(); acc.setflags(write=False)
        _oracle[key] = (acc, orc.resolve(ref, spp), spp, cnt.rays)
    return _oracle[key]


_gpu = {}


def gpu_frame(art, backend, name, rt, frame, depth, per, vthreads=1, batch_paths=DEFAULT_BATCH_PATHS):
    """One render with shade_per = per set before the upload, the resize and the pass; rendered once per (case, per) and kept, so that the
    test of the other value compares its LDR frame with this one.  (accum bits, LDR frame, spp, rays, samples, batches)"""
    key = (name, rt, frame, depth, per, vthreads, batch_paths)
    if key not in _gpu:
        w, h, aa = FRAMES[frame]
        backend.set_option("shade_per", per)
        backend.set_option("batch_paths", batch_paths)
        try:
            backend.upload_scene(scene(art, name)[0])
            backend.resize(w, h)
            accum, screen, spp = backend.render_pass(art.Backend.pass_params(getattr(art, rt), aa, depth, vthreads, seed=SEED), 0, want_screen=True)
            st = backend.stats()
            assert st.lost_paths == 0
            _gpu[key] = (bits(accum).copy(), screen.copy(), spp, st.rays, st.samples, backend.stage_stats().batches)
        finally:
            backend.set_option("shade_per", 0)
            backend.set_option("batch_paths", DEFAULT_BATCH_PATHS)
    return _gpu[key]


def check_case(art, backend, name, rt, frame, depth, per):
    acc, screen, spp, rays = oracle_frame(art, name, rt, frame, depth)
    w, h, aa = FRAMES[frame]
    assert spp == (4 if aa else 1)
    got = gpu_frame(art, backend, name, rt, frame, depth, per)
    print("%s %s %s depth %d shade_per %d: %d paths, rays %d (oracle %d), %d accum words differ" % (name, rt, frame, depth, per, w * h * spp, got[3], rays, int((got[0] != acc).sum())))
    assert got[2] == spp and got[4] == w * h * spp and got[5] == 1
    assert np.array_equal(got[0], acc), "accum differs from the oracle's in %d of %d words" % (int((got[0] != acc).sum()), acc.size)
    assert got[3] == rays
    assert np.array_equal(got[1], screen)
    other = gpu_frame(art, backend, name, rt, frame, depth, PERS[1 - PERS.index(per)])
    assert np.array_equal(got[1], other[1]), "the LDR frame depends on shade_per"


def first_hit_types(art, name, frame):
    """Material types (art.MAT_*) among the closest hits of the frame's camera rays through the pixel centres (ray_tracer.adb:61-69),
    by the oracle, and the number of rays that hit nothing"""
    sd = scene(art, name)[2]
    w, h, _ = FRAMES[frame]
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    d = np.stack([x + 0.5 - w / 2.0, y + 0.5 - h / 2.0, np.full_like(x, -float(w))], -1).reshape(-1, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.tile(np.array(list(sd.desc.cam_pos), np.float32), (d.shape[0], 1))
    hits = orc.closest_hits(scene(art, name)[1].scene, o, d)
    types = {sd.desc.materials[h.mat].type for h in hits if h.is_hit}
    return types, sum(1 for h in hits if not h.is_hit)


def scene_material_types(art, name):
    """the material types some primitive of the scene carries: spheres, the box's walls, mesh triangles"""
    d = scene(art, name)[2].desc
    ids = {d.spheres[i].mat for i in range(d.n_spheres)} | (set(d.cb_mat) if d.has_cornell else set())
    for i in range(d.n_meshes):
        ids |= set(np.ctypeslib.as_array(d.meshes[i].matid, (d.meshes[i].ntris,)).tolist())
    return {d.materials[m].type for m in ids}


# ---- the reference's own scene: no BVH, every integrator, every frame ------------------------------------------------------------------
@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("frame", ["1x1", "16x8", "23x11", "23x11-noaa", "33x16"])
@pytest.mark.parametrize("rt", INTEGRATORS)
def test_reference_scene(art, backend, rt, frame, per):
    check_case(art, backend, "cornell", rt, frame, 8, per)


# ---- every material next to every other: more than two classes in a round of the class sort -----------------------------------------------
@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("frame", ["33x16", "23x11"])
@pytest.mark.parametrize("rt", INTEGRATORS)
@pytest.mark.parametrize("name", ["mixed", "mirror"])
def test_mixed_and_mirror_scenes(art, backend, name, rt, frame, per):
    """The classes the sort separates are all there: every material type of the scene is the first hit of some camera ray of the frame,
    and some camera rays hit nothing."""
    types, misses = first_hit_types(art, name, frame)
    want = scene_material_types(art, name)
    assert want >= ({art.MAT_GLASS, art.MAT_LAMBERT, art.MAT_LIGHT, art.MAT_PHONG} | ({art.MAT_MIRROR} if name == "mirror" else set()))
    assert types == want, "material types among the first hits %s, in the scene %s" % (sorted(types), sorted(want))
    assert misses > 0
    check_case(art, backend, name, rt, frame, 8, per)


# ---- depths 1, 2 and 8, sphere and rect lights --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("depth", [1, 2, 8])
@pytest.mark.parametrize("name", ["synthetic", "rect"])
def test_depths_and_rect_lights(art, backend, name, depth, per):
    """Depth 1: the CAMERA instantiation is also the last stage and writes shadow records only.  Rect lights: the NaN pixels of
    test_gpu_parity.test_rect_light_mis_nan_pattern_matches (the bit comparison holds their positions and payloads too)."""
    acc = oracle_frame(art, name, "PT_MIS", "33x16", depth)[0]
    assert bool(np.isnan(acc.view(np.float32)).any()) == (name == "rect")
    check_case(art, backend, name, "PT_MIS", "33x16", depth, per)


# ---- the scene's own tables instead of the LDS copies ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", PERS)
def test_more_spheres_and_lights_than_lds_holds(art, backend, per):
    check_case(art, backend, "lds", "PT_MIS", "23x11", 8, per)


# ---- an instanced scene against the oracle on its flattened copy ------------------------------------------------------------------------------
@pytest.mark.parametrize("per", PERS)
def test_instanced_scene(art, backend, per):
    check_case(art, backend, "instanced", "PT_MIS", "33x16", 8, per)


# ---- several batches at a pinned value ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("vthreads", [2, 3])
def test_several_batches_at_a_pinned_value(art, backend, vthreads, per):
    """32x16, batch_paths = 1024: 256 pixels x 4 samples per batch (test_gpu_batch_shape.plan), so 2 x 2 batches for 8 samples and 2 x 3
    for the 12 of vthreads = 3 -- every one of them with the pinned value.  The frame of the same pass in one batch, and the oracle's."""
    S = 4 * vthreads
    acc, screen, spp, rays = oracle_frame(art, "synthetic", "PT_MIS", "32x16", 8, vthreads)
    one = gpu_frame(art, backend, "synthetic", "PT_MIS", "32x16", 8, per, vthreads)
    got = gpu_frame(art, backend, "synthetic", "PT_MIS", "32x16", 8, per, vthreads, batch_paths=1024)
    print("vthreads %d shade_per %d: batches %d / %d, rays %d / %d (oracle %d)" % (vthreads, per, one[5], got[5], one[3], got[3], rays))
    assert one[5] == 1 and got[5] == 2 * (S // 4)
    assert got[2] == one[2] == spp == S and got[4] == one[4] == 32 * 16 * S
    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]) and got[3] == one[3]
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], screen) and got[3] == rays


# ---- the trial itself -------------------------------------------------------------------------------------------------------------------------------
def test_the_trial_gives_the_pinned_frames(art, backend):
    """shade_per = 0 (the default), 32x24, 8 samples, batch_paths = 1024: six batches of 256 pixels x 4 samples.  Batches 1 and 2 run 4
    items per thread (warm, trial A), batch 3 runs 2 (trial B: the same number of paths as trial A), batches 4 to 6 run 4 until a call
    that waits has read the trials' events and the measured choice afterwards: WHICH VALUE BATCHES 4 ONWARD RUN IS THE ONLY
    TIMING-DEPENDENT PART of this test, and either value must give the same frame.  The frame is the pinned frames' (one batch each)
    and the oracle's, and the counters are equal."""
    acc, screen, spp, rays = oracle_frame(art, "synthetic", "PT_MIS", "32x24", 8, 2)
    pinned = [gpu_frame(art, backend, "synthetic", "PT_MIS", "32x24", 8, per, 2) for per in PERS]
    got = gpu_frame(art, backend, "synthetic", "PT_MIS", "32x24", 8, 0, 2, batch_paths=1024)
    print("trial: batches %d, rays %d (pinned %d, %d; oracle %d)" % (got[5], got[3], pinned[0][3], pinned[1][3], rays))
    assert got[5] == 6 and pinned[0][5] == pinned[1][5] == 1
    for p in pinned:
        assert np.array_equal(got[0], p[0]) and np.array_equal(got[1], p[1])
        assert (got[2], got[3], got[4]) == (p[2], p[3], p[4])
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], screen) and (got[2], got[3]) == (spp, rays)
