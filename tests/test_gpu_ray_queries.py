"""Device-resident ray queries (art_trace_rays_device / art_occluded_rays_device through Backend.trace_rays_torch / occluded_torch):
the same 44 bytes per ray as art_trace_rays, the tnear / tfar rule of gcore's run_batch, occlusion == is_hit, slicing, stream order
and refusal of bad inputs before any launch."""
import ctypes as C

import numpy as np
import pytest

import conv
import orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
FLT_MAX = np.float32(3.4028234663852886e38)
art_LIGHT_SPHERE = 1


def _scene(art, name):
    from ada_ray_tracer_amd import scenes
    if name == "synthetic":
        return scenes.synthetic_scene(2000, 3), True          # Cornell walls + random triangles + 3 sphere lights (spheres)
    if name == "rect":
        return scenes.synthetic_scene(2000, 3, rect_lights=True), True     # quad lights
    if name == "reference":
        return scenes.reference_scene(), False                 # the reference's scene: REFERENCE_BF pyramid, spheres, Cornell box
    return scenes.instanced_scene(n_instances=8, tris_per_mesh=2000), True


SCENES = ["synthetic", "rect", "reference", "instanced"]


def _rays(n, seed):
    """Random rays inside and outside the box, axis-parallel directions among them, and rays that leave the scene (misses)."""
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2]).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    k = n // 8
    axes = np.eye(3, dtype=np.float32)
    d[:k] = axes[rng.integers(0, 3, k)] * rng.choice(np.float32([-1.0, 1.0]), (k, 1))     # exactly axis-parallel
    d[k:2 * k, rng.integers(0, 3)] = 0.0                                                    # one zero component
    o[2 * k:3 * k] = np.float32([0.0, 2.5, 40.0]) + (rng.random((k, 3)) - 0.5).astype(np.float32)   # far outside the box ...
    d[2 * k:3 * k, 2] = np.abs(d[2 * k:3 * k, 2])                                           # ... looking away from it: misses
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def _with_surface_starts(backend, o, d):
    """Half of the hitting rays restarted at their hit point (rays that start on surfaces)."""
    h = conv.hits_to_arrays(backend.trace_rays(o, d))
    hit = np.nonzero(h[1] == 1)[0][::2]
    o2 = o.copy()
    o2[hit] = o[hit] + h[0][hit][:, None] * d[hit]
    return o2, d


def _host_raw(hits):
    return np.frombuffer(C.string_at(C.addressof(hits), C.sizeof(hits)), np.int32).reshape(-1, 11)


def _gpu(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _assert_same_bytes(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%d of %d records differ, first %d: got %s want %s" % (bad.size, len(want), bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("scene", SCENES)
def test_closest_hit_bytes_equal_art_trace_rays(art, backend, scene):
    sd, _ = _scene(art, scene)
    backend.upload_scene(sd)
    o, d = _with_surface_starts(backend, *_rays(30000, 11))
    og, dg = _gpu(o, d)
    for kernel in (art.TRACE_COOP, art.TRACE_SIMPLE):
        want = _host_raw(backend.trace_rays(o, d, kernel=kernel))
        assert (want[:, 1] == 1).any() and (want[:, 1] == 0).any()
        _assert_same_bytes(backend.trace_rays_torch(og, dg, kernel=kernel).raw, want)


def _interval_case(n, seed):
    rng = np.random.default_rng(seed)
    tn = (rng.random(n) * 3.0 - 0.5).astype(np.float32)            # negative, zero and positive tnear
    tn[::7] = 0.0
    tf = (tn + rng.random(n) * 6.0 - 0.5).astype(np.float32)        # some intervals empty (tfar <= tnear)
    tf[::11] = tn[::11]                                             # tfar == tnear: empty
    tf[::13] = FLT_MAX
    return tn, tf


def _expected_with_interval(backend, o, d, tn, tf, kernel):
    """gcore_api.cpp run_batch in numpy float32: shift, art_trace_rays on the live rays, t0 added back to hits; empty intervals miss."""
    t0 = np.where(tn > 0, tn, np.float32(0.0)).astype(np.float32)
    os_ = (o + t0[:, None] * d).astype(np.float32)
    f = (tf - t0).astype(np.float32)
    live = f > 0
    want = np.zeros((len(o), 11), np.int32)
    want[:, 0] = f.view(np.int32); want[:, 2:6] = -1                 # the miss record: t = the bound, u = v = 0
    idx = np.nonzero(live)[0]
    sub = _host_raw(backend.trace_rays(np.ascontiguousarray(os_[idx]), np.ascontiguousarray(d[idx]), np.ascontiguousarray(f[idx]), kernel=kernel)).copy()
    h = sub[:, 1] == 1
    sub[h, 0] = (t0[idx][h] + sub[h, 0].view(np.float32)).astype(np.float32).view(np.int32)
    want[idx] = sub
    return want, os_, live


@pytest.mark.parametrize("scene", SCENES)
def test_tnear_tfar_follow_the_gcore_rule(art, backend, scene):
    sd, _ = _scene(art, scene)
    backend.upload_scene(sd)
    o, d = _rays(20000, 23)
    tn, tf = _interval_case(len(o), 5)
    og, dg, tng, tfg = _gpu(o, d, tn, tf)
    for kernel in (art.TRACE_COOP, art.TRACE_SIMPLE):
        want, _, live = _expected_with_interval(backend, o, d, tn, tf, kernel)
        assert (~live).sum() > 1000 and (want[:, 1] == 1).sum() > 1000
        got = backend.trace_rays_torch(og, dg, tng, tfg, kernel=kernel)
        _assert_same_bytes(got.raw, want)
        assert not got.is_hit.cpu().numpy()[~live].any()
    # tnear only (tfar NULL = Float'Last): against art_trace_rays and against the oracle on the shifted rays
    want, os_, _ = _expected_with_interval(backend, o, d, tn, np.full(len(o), FLT_MAX, np.float32), art.TRACE_COOP)
    got = backend.trace_rays_torch(og, dg, tnear=tng)
    _assert_same_bytes(got.raw, want)
    if scene in ("synthetic", "reference"):
        osc = orc.CornellScene().scene if scene == "reference" else conv.OracleScene(sd).scene
        oh = conv.hits_to_arrays(orc.closest_hits(osc, os_, d))
        t0 = np.where(tn > 0, tn, np.float32(0.0)).astype(np.float32)
        ref_t = (t0 + oh[0]).astype(np.float32)
        hit = oh[1] == 1
        assert np.array_equal(got.is_hit.cpu().numpy(), oh[1])
        assert np.array_equal(got.prim_type.cpu().numpy(), oh[2])
        assert np.array_equal(got.t.cpu().numpy()[hit].view(np.uint32), ref_t[hit].view(np.uint32))
        assert np.array_equal(got.prim_index.cpu().numpy()[hit], oh[3][hit])
        assert np.array_equal(got.mat.cpu().numpy()[hit], oh[4][hit])
        assert np.array_equal(got.normal.cpu().numpy()[hit].view(np.uint32), oh[5][hit].view(np.uint32))


def _shadow_rays(backend, sd, n, seed):
    """Surface points towards samples on the lights: tfar = the distance to the sample, a small tnear."""
    rng = np.random.default_rng(seed)
    o, d = _rays(n, seed)
    h = conv.hits_to_arrays(backend.trace_rays(o, d))
    hit = np.nonzero(h[1] == 1)[0]
    p = (o[hit] + h[0][hit][:, None] * d[hit]).astype(np.float32)
    return _shadow_rays_from(sd, p, rng)


def _shadow_rays_from(sd, p, rng):
    """The shadow rays of the surface points p [m, 3] (float32), wherever they come from."""
    L = sd.desc.lights
    samples = []
    for i in range(sd.desc.n_lights):
        if L[i].shape == art_LIGHT_SPHERE:                               # sphere light: a point just outside it, on the side that faces p
            c = np.array(L[i].center, np.float32)
            u = (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True) + (rng.random((len(p), 3)) - 0.5) * 0.6
            samples.append((c + u / np.linalg.norm(u, axis=1, keepdims=True) * (1.5 * L[i].radius)).astype(np.float32))
        else:                                                            # rect light: a point of its box
            lo, hi = np.array(L[i].boxMin, np.float32), np.array(L[i].boxMax, np.float32)
            samples.append((lo + rng.random((len(p), 3)) * (hi - lo)).astype(np.float32))
    s = np.stack(samples)[rng.integers(0, len(samples), len(p)), np.arange(len(p))]
    v = (s - p).astype(np.float32)
    dist = np.linalg.norm(v, axis=1).astype(np.float32)
    sd_ = (v / dist[:, None]).astype(np.float32)
    return p, sd_, np.full(len(p), 1e-4, np.float32), (dist * np.float32(0.999)).astype(np.float32)


@pytest.mark.parametrize("scene", SCENES)
def test_occlusion_equals_is_hit(art, backend, scene):
    sd, _ = _scene(art, scene)
    backend.upload_scene(sd)
    o, d = _with_surface_starts(backend, *_rays(30000, 31))
    tn, tf = _interval_case(len(o), 9)
    og, dg, tng, tfg = _gpu(o, d, tn, tf)
    for args in ((og, dg, None, None), (og, dg, tng, tfg), (og, dg, None, tfg)):
        want = backend.trace_rays_torch(*args).is_hit.cpu().numpy() != 0
        got = backend.occluded_torch(*args).cpu().numpy()
        assert got.dtype == np.bool_ and np.array_equal(got, want)
    p, sdir, stn, stf = _shadow_rays(backend, sd, 40000, 37)
    pg, sg, stng, stfg = _gpu(p, sdir, stn, stf)
    want = backend.trace_rays_torch(pg, sg, stng, stfg).is_hit.cpu().numpy() != 0
    got = backend.occluded_torch(pg, sg, stng, stfg).cpu().numpy()
    assert want.any() and not want.all(), want.mean()                # both answers occur
    assert np.array_equal(got, want)


def test_slices_give_the_same_bytes(art, backend):
    sd, _ = _scene(art, "synthetic")
    backend.upload_scene(sd)
    o, d = _rays(10007, 41)
    tn, tf = _interval_case(len(o), 43)
    args = _gpu(o, d, tn, tf)
    whole = {k: backend.trace_rays_torch(*args, kernel=k).raw.cpu().numpy() for k in (art.TRACE_COOP, art.TRACE_SIMPLE)}
    occ = backend.occluded_torch(*args).cpu().numpy()
    backend.set_option("query_slice", 1000)
    try:
        for k in (art.TRACE_COOP, art.TRACE_SIMPLE):
            _assert_same_bytes(backend.trace_rays_torch(*args, kernel=k).raw, whole[k])
        assert np.array_equal(backend.occluded_torch(*args).cpu().numpy(), occ)
    finally:
        backend.set_option("query_slice", 1 << 24)


def test_queries_on_a_side_stream(art, backend):
    """A query on a non-default torch stream, consumed on that stream; and render passes around queries that run on another stream
    keep their accum bits."""
    sd, _ = _scene(art, "synthetic")
    backend.upload_scene(sd)
    o, d = _rays(50000, 53)
    want = _host_raw(backend.trace_rays(o, d))
    og, dg = _gpu(o, d)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h = backend.trace_rays_torch(og, dg)
        t2 = h.t * 2.0                                                 # consumed on the same stream, no synchronise in between
        occ = backend.occluded_torch(og, dg).to(torch.int32) * 3
    s.synchronize()
    _assert_same_bytes(h.raw, want)
    with np.errstate(over="ignore"):                                  # (misses hold Float'Last: twice that is inf on both sides)
        assert np.array_equal(t2.cpu().numpy(), (want[:, 0].view(np.float32) * np.float32(2.0)).astype(np.float32))
    assert np.array_equal(occ.cpu().numpy(), (want[:, 1] != 0).astype(np.int32) * 3)

    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=7)
    backend.resize(48, 48)
    spp = backend.render_pass_device(p, 0)
    plain, _, _ = backend.render_pass(p, spp)
    backend.resize(48, 48)
    spp = backend.render_pass_device(p, 0)                             # enqueued, not waited for
    with torch.cuda.stream(s):
        q1 = backend.trace_rays_torch(og, dg)
        q2 = backend.occluded_torch(og, dg)
    mixed, _, _ = backend.render_pass(p, spp)
    with torch.cuda.stream(s):
        q3 = backend.trace_rays_torch(og, dg, kernel=art.TRACE_SIMPLE)
    s.synchronize()
    assert np.array_equal(mixed.view(np.uint32), plain.view(np.uint32))
    _assert_same_bytes(q1.raw, want)
    _assert_same_bytes(q3.raw, want)
    assert np.array_equal(q2.cpu().numpy(), want[:, 1] != 0)


def test_bad_inputs_are_refused_before_any_launch(art, backend):
    sd, _ = _scene(art, "synthetic")
    backend.upload_scene(sd)
    o, d = _rays(64, 61)
    og, dg = _gpu(o, d)
    for call in (backend.trace_rays_torch, backend.occluded_torch):
        with pytest.raises(art.ArtError, match="GPU tensor"):
            call(torch.from_numpy(o), dg)                                   # a CPU tensor
        with pytest.raises(art.ArtError, match="GPU tensor"):
            call(og, dg, tfar=torch.ones(64))                               # a CPU interval
        with pytest.raises(art.ArtError, match="float32"):
            call(og.double(), dg)
        with pytest.raises(art.ArtError, match="shape"):
            call(og, dg[:63])
        with pytest.raises(art.ArtError, match="shape"):
            call(og, dg, tnear=torch.zeros(65, device="cuda"))
    # non-contiguous inputs are made contiguous, not refused
    big = torch.cat([og, dg], dim=1)
    _assert_same_bytes(backend.trace_rays_torch(big[:, :3], big[:, 3:]).raw, _host_raw(backend.trace_rays(o, d)))
    # the C ABI: host memory is refused by hipPointerGetAttributes before anything is launched
    L = backend.lib
    out = np.zeros((64, 11), np.int32)
    host = lambda a: a.ctypes.data
    assert L.art_trace_rays_device(host(o), host(d), None, None, 64, host(out), art.TRACE_COOP, None) != 0
    assert "not device memory" in L.art_last_error().decode()
    raw = torch.empty((64, 11), dtype=torch.int32, device="cuda")
    assert L.art_trace_rays_device(og.data_ptr(), host(d), None, None, 64, raw.data_ptr(), art.TRACE_COOP, None) != 0
    assert "dirs" in L.art_last_error().decode()
    assert L.art_occluded_rays_device(og.data_ptr(), dg.data_ptr(), None, None, 64, host(out), None) != 0
    assert "occluded_out" in L.art_last_error().decode()
    assert L.art_trace_rays_device(og.data_ptr(), dg.data_ptr(), None, None, 64, raw.data_ptr(), 7, None) != 0
    assert "unknown kernel" in L.art_last_error().decode()
    assert L.art_trace_rays_device(og.data_ptr(), dg.data_ptr(), None, None, 1 << 31, raw.data_ptr(), art.TRACE_COOP, None) != 0
    # the library still answers afterwards
    _assert_same_bytes(backend.trace_rays_torch(og, dg).raw, _host_raw(backend.trace_rays(o, d)))


def test_queries_between_passes_leave_the_context_alone(art, backend):
    """Queries name their own stream and kernel; the context keeps its own.  Between two render passes: a sliced closest-hit query with the
    one-ray-per-lane kernel on a side stream (1000 rays in slices of 256: four slices, the last one partial), an occlusion query, and a
    query that is refused.  The second pass still renders on the context's stream with the context's kernel: the picture has the bits of
    two passes without queries, the hits are those of the cooperative kernel, and only the passes' launches are timed."""
    from ada_ray_tracer_amd import scenes
    depth = 3
    backend.upload_scene(scenes.mirror_scene())                       # 600 triangles behind the BVH, every material
    o, d = _rays(1000, 71)
    og, dg = _gpu(o, d)
    p = art.Backend.pass_params(art.PT_MIS, True, depth, 1, seed=7)   # 4 samples per pass
    backend.resize(64, 64)
    spp = backend.render_pass_device(p, 0)
    plain, _, _ = backend.render_pass(p, spp)
    coop = backend.trace_rays_torch(og, dg, kernel=art.TRACE_COOP).raw.cpu().numpy()
    assert (coop[:, 1] == 1).any() and (coop[:, 1] == 0).any()
    torch.cuda.synchronize()

    backend.resize(64, 64)
    spp = backend.render_pass_device(p, 0)
    s = torch.cuda.Stream()
    L = backend.lib
    backend.set_option("query_slice", 256)
    try:
        with torch.cuda.stream(s):
            simple = backend.trace_rays_torch(og, dg, kernel=art.TRACE_SIMPLE)
            occ = backend.occluded_torch(og, dg)
        raw = torch.empty((1000, 11), dtype=torch.int32, device="cuda")
        assert L.art_trace_rays_device(o.ctypes.data, dg.data_ptr(), None, None, 1000, raw.data_ptr(), art.TRACE_SIMPLE, s.cuda_stream) != 0
        assert "origins is not device memory" in L.art_last_error().decode()
    finally:
        backend.set_option("query_slice", 1 << 24)
    mixed, _, _ = backend.render_pass(p, spp)
    s.synchronize()
    assert np.array_equal(mixed.view(np.uint32), plain.view(np.uint32))
    _assert_same_bytes(simple.raw, coop)
    assert np.array_equal(occ.cpu().numpy(), coop[:, 1] != 0)
    # one camera trace plus one trace per bounce, one shade per bounce, one batch per pass; the untimed query launches add nothing
    st, stage = backend.stats(), backend.stage_stats()
    assert st.trace_launches == 2 * (1 + depth), st.trace_launches
    assert stage.shade_launches == 2 * depth and stage.batches == 2, (stage.shade_launches, stage.batches)
