"""Moving geometry (art_refit_device through Backend.refit_torch): a refit of the unmoved mesh reproduces the uploaded tree byte for byte,
a refitted scene answers queries and renders exactly like a fresh upload of the moved mesh, the refitted tree is sound, refits are
stream-ordered, every context of art_init_devices is refitted, and bad input is refused or reported without a hang."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

import bvh_check
import conv

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32


def _scene(name):
    from ada_ray_tracer_amd import scenes
    return scenes.synthetic_scene(2000, 3) if name == "synthetic" else scenes.structured_scene(20000)


def _mesh(sd):
    pos, nrm, idx, _, matid = sd._mesh_arrays[-1]
    return pos, nrm, idx, matid


def _moved(art, sd, pos, nrm):
    """A fresh scene description: sd with its CLOSEST mesh at new positions / normals (same indices, same material ids)."""
    _, _, idx, matid = _mesh(sd)
    return art.SceneDesc(meshes=[dict(mode=art.MESH_CLOSEST, pos=pos, nrm=nrm, idx=idx, matid=matid)], **sd._kw)


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _deform(name, pos, nrm, seed=1, amount=1.0):
    """structured: the mesh rotated about its centre, a smooth displacement and a small jitter; synthetic: the soup translated."""
    p64 = pos.astype(np.float64); n64 = nrm.astype(np.float64)
    if name == "synthetic":
        return (p64 + amount * np.array([0.11, -0.07, 0.23])).astype(F), nrm.copy()
    rng = np.random.default_rng(seed)
    c = p64.mean(0)
    R = _rot_y(0.3 * amount)
    p = (p64 - c) @ R.T + c
    p[:, 1] += amount * 0.08 * np.sin(3.0 * p[:, 0]) * np.cos(2.0 * p[:, 2])
    p += amount * 1e-3 * rng.standard_normal(p.shape)
    return p.astype(F), (n64 @ R.T).astype(F)


def _rays(n, seed):
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2]).astype(F)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    k = n // 8
    d[:k] = np.eye(3, dtype=F)[rng.integers(0, 3, k)] * rng.choice(F([-1.0, 1.0]), (k, 1))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def _with_surface_starts(backend, o, d):
    h = conv.hits_to_arrays(backend.trace_rays(o, d))
    hit = np.nonzero(h[1] == 1)[0][::2]
    o2 = o.copy()
    o2[hit] = o[hit] + h[0][hit][:, None] * d[hit]
    return o2, d


def _gpu(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _host_raw(hits):
    return np.frombuffer(C.string_at(C.addressof(hits), C.sizeof(hits)), np.int32).reshape(-1, 11)


def _export(backend):
    nodes, tris, info = backend.export_bvh()
    return nodes.view(np.uint32).copy(), tris.view(np.uint32).copy(), info


def _observe(art, backend, o, d):
    """What a caller sees of the scene: closest-hit bytes of both kernels (GPU tensors) and of art_trace_rays (host arrays), occlusion,
    and a 4-spp PT_MIS frame (accum bits, screen, rays)."""
    og, dg = _gpu(o, d)
    out = {}
    for k in (art.TRACE_COOP, art.TRACE_SIMPLE):
        out["hits%d" % k] = backend.trace_rays_torch(og, dg, kernel=k).raw.cpu().numpy()
    out["host"] = _host_raw(backend.trace_rays(o, d)).copy()
    out["occ"] = backend.occluded_torch(og, dg).cpu().numpy()
    backend.resize(96, 96)
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=3)
    accum, screen, spp = backend.render_pass(p, 0, True, True)
    assert spp == 4
    out["accum"] = accum.view(np.uint32); out["screen"] = screen; out["rays"] = np.array([backend.stats().rays])
    return out


def _assert_same(got, want):
    for k in want:
        assert np.array_equal(got[k], want[k]), "%s differs in %d places" % (k, int((got[k] != want[k]).sum()))


@pytest.fixture
def options(backend):
    """Options set by a test are put back to the defaults afterwards (the session's backend is shared)."""
    yield backend.set_option
    for name, value in (("bvh_width", 4), ("bvh_builder", 3), ("bvh_spatial_splits", 0)):
        backend.set_option(name, value)


def _refit(backend, pos, nrm=None, check=True):
    pg, ng = _gpu(pos, nrm)
    backend.refit_torch(pg, ng, check=check)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["synthetic", "structured"])
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("builder", [3, 0, 1, 2])
def test_identity_refit_reproduces_the_uploaded_tree(art, backend, options, name, width, builder):
    sd = _scene(name)
    options("bvh_width", width); options("bvh_builder", builder)
    backend.upload_scene(sd)
    n0, t0, i0 = _export(backend)
    pos, nrm, _, _ = _mesh(sd)
    _refit(backend, pos)
    n1, t1, i1 = _export(backend)
    assert (i1.n_nodes, i1.n_tris, i1.max_stack, i1.node_width) == (i0.n_nodes, i0.n_tris, i0.max_stack, width)
    assert np.array_equal(t1, t0), "triangle records differ"
    assert np.array_equal(n1, n0), "%d of %d node words differ" % (int((n1 != n0).sum()), n0.size)
    ri = backend.refit_info()
    assert ri.refits == 1 and ri.bad_vertices == 0 and ri.plan_ms > 0.0 and ri.refit_ms > 0.0


@pytest.mark.parametrize("name", ["structured", "synthetic"])
@pytest.mark.parametrize("with_nrm", [True, False])
def test_moved_mesh_equals_a_fresh_upload(art, backend, name, with_nrm):
    sd = _scene(name)
    pos, nrm, _, _ = _mesh(sd)
    p2, n2 = _deform(name, pos, nrm)
    backend.upload_scene(_moved(art, sd, p2, n2 if with_nrm else nrm))
    o, d = _with_surface_starts(backend, *_rays(30000, 7))
    want = _observe(art, backend, o, d)
    assert (want["hits0"][:, 1] == 1).sum() > 10000 and want["occ"].any() and not want["occ"].all()
    assert (want["hits0"][:, 2] == 2).sum() > 1000                       # (prim_type 2: triangle hits -- the moved mesh is actually hit)
    backend.upload_scene(sd)
    before = _observe(art, backend, o, d)
    assert not np.array_equal(before["accum"], want["accum"])            # the deformation shows in the picture
    _refit(backend, p2, n2 if with_nrm else None)
    _assert_same(_observe(art, backend, o, d), want)


@pytest.mark.parametrize("builder,width,splits", [(3, 4, 0), (0, 4, 0), (1, 4, 0), (2, 8, 0), (0, 4, 1), (0, 8, 1)])
def test_refitted_tree_is_sound(art, backend, options, builder, width, splits):
    sd = _scene("structured")
    options("bvh_width", width); options("bvh_builder", builder); options("bvh_spatial_splits", splits)
    backend.upload_scene(sd)
    pos, nrm, idx, _ = _mesh(sd)
    p2, n2 = _deform("structured", pos, nrm, amount=2.0)
    _refit(backend, p2, n2)
    nodes, tris, info = backend.export_bvh()
    bvh_check.check_tree(nodes, tris, info.n_nodes, info.max_stack, width, p2, idx, allow_duplicates=bool(splits))


@pytest.mark.parametrize("builder,width", [(3, 4), (0, 8)])
def test_round_trip_restores_the_tree(art, backend, options, builder, width):
    sd = _scene("structured")
    options("bvh_width", width); options("bvh_builder", builder)
    backend.upload_scene(sd)
    n0, t0, _ = _export(backend)
    pos, nrm, _, _ = _mesh(sd)
    p1, n1 = _deform("structured", pos, nrm, seed=2)
    p2, n2 = _deform("structured", p1, n1, seed=3, amount=-0.5)
    for p, n in ((p1, n1), (p2, n2), (pos, nrm)):
        _refit(backend, p, n)
    n3, t3, _ = _export(backend)
    assert np.array_equal(t3, t0) and np.array_equal(n3, n0)
    assert backend.refit_info().refits == 3


def test_refit_is_stream_ordered(art, backend):
    sd = _scene("structured")
    pos, nrm, _, _ = _mesh(sd)
    p2, _ = _deform("structured", pos, nrm)
    o, d = _rays(30000, 9)
    og, dg = _gpu(o, d)
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=5)
    backend.upload_scene(_moved(art, sd, p2, nrm))
    want_new = backend.trace_rays_torch(og, dg).raw.cpu().numpy()
    backend.resize(64, 64)
    new_img, _, _ = backend.render_pass(p, 0)
    backend.upload_scene(sd)
    want_old = backend.trace_rays_torch(og, dg).raw.cpu().numpy()
    backend.resize(64, 64)
    old_img, _, _ = backend.render_pass(p, 0)
    assert not np.array_equal(want_old, want_new)
    pg = _gpu(p2)[0]
    torch.cuda.synchronize()
    backend.resize(64, 64)
    spp = backend.render_pass_device(p, 0)                               # enqueued on the library's stream, not waited for
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h1 = backend.trace_rays_torch(og, dg)
        backend.refit_torch(pg, check=False)                             # (check=False: no host synchronisation in between)
        h2 = backend.trace_rays_torch(og, dg)
    accum, _ = backend.download(spp, want_screen=False)                  # the pass enqueued before the refit: the old geometry
    s.synchronize()
    assert np.array_equal(h1.raw.cpu().numpy(), want_old)
    assert np.array_equal(h2.raw.cpu().numpy(), want_new)
    assert np.array_equal(accum.view(np.uint32), old_img.view(np.uint32))
    backend.resize(64, 64)
    img, _, _ = backend.render_pass(p, 0)                                # enqueued after it: the new geometry
    assert np.array_equal(img.view(np.uint32), new_img.view(np.uint32))


SCRIPT = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import torch
import ctypes as C
import test_gpu_refit as T
out = {}
sd = T._scene("structured")
pos, nrm, idx, _ = T._mesh(sd)
p2, n2 = T._deform("structured", pos, nrm)
p = art.Backend.pass_params(art.PT_MIS, True, 8, 2, seed=5)
be = art.Backend(0)
try:
    be.refit_torch(torch.from_numpy(pos).cuda())
    out["no_scene"] = "accepted"
except art.ArtError as e:
    out["no_scene"] = str(e)
L = be.lib
verts = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0); tri = (C.c_int * 3)(0, 1, 2)
L.gcore_init_and_clear()
L.gcore_instance_meshes(L.gcore_add_mesh_3f(verts, 3, tri, 3), (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1), 1)
L.gcore_commit_scene()
try:
    be.refit_torch(torch.zeros((3, 3), device="cuda"))
    out["gcore"] = "accepted"
except art.ArtError as e:
    out["gcore"] = str(e)
L.gcore_destroy()
be.upload_scene(T._moved(art, sd, p2, n2)); be.resize(100, 72)
accum, screen, spp = be.render_pass(p, 0, True, True)
ref = (accum.copy(), screen.copy(), spp, be.stats().rays)
be.shutdown()
for builder in (1, 3):
    be = art.Backend(devices=[0, 0, 0])
    be.set_option("bvh_builder", builder)                    # (1: every context builds its own LBVH)
    be.upload_scene(sd); be.resize(100, 72)
    be.render_pass(p, 0, True, True)                         # (the old geometry rendered once on every context)
    be.refit_torch(torch.from_numpy(p2).cuda(), torch.from_numpy(n2).cuda())
    be.resize(100, 72)
    accum, screen, spp = be.render_pass(p, 0, True, True)
    out["three_contexts_builder%d" % builder] = bool(np.array_equal(accum.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(screen, ref[1])
                                                   and spp == ref[2] and be.stats().rays == ref[3])
    out["refits_%d" % builder] = be.refit_info().refits
    be.shutdown()
print("RESULT " + json.dumps(out))
'''


def test_contexts_on_one_gpu_are_all_refitted(art):
    """art_init_devices([0, 0, 0]) in a child process (the library is a process-wide singleton), plus the refusals that need a fresh
    process: no scene yet, and a scene committed through the gcore seam."""
    r = subprocess.run([sys.executable, "-c", SCRIPT, art.ROOT], capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(line[0][7:])
    assert "no scene uploaded" in out["no_scene"]
    assert "gcore_commit_scene" in out["gcore"]
    assert out["three_contexts_builder1"] and out["three_contexts_builder3"]
    assert out["refits_1"] == 1 and out["refits_3"] == 1


def _many_refits(art, be, width, n=200):
    """The synthetic mesh uploaded at P, then n refits back to back on a side stream with nothing waited for in between -- alternately
    to a deformed mesh and to P, the last one at P -- and ONE synchronize.  Returns ArtRefitInfo's figures and whether the exported tree
    equals the fresh upload's."""
    sd = _scene("synthetic")
    pos, nrm, _, _ = _mesh(sd)
    p2, _ = _deform("synthetic", pos, nrm)
    be.set_option("bvh_width", width)
    be.upload_scene(sd)
    n0, t0, _ = _export(be)
    g = _gpu(p2, pos)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        for k in range(n):
            be.refit_torch(g[k % 2], check=False)
    be.synchronize()
    ri = be.refit_info()
    n1, t1, _ = _export(be)
    return dict(refits=int(ri.refits), refit_ms=float(ri.refit_ms), bad_vertices=int(ri.bad_vertices),
                nodes_equal=bool(np.array_equal(n1, n0)), tris_equal=bool(np.array_equal(t1, t0)))


def _check_many_refits(out, n=200):
    print("many refits:", out)
    assert out["refits"] == n
    assert out["refit_ms"] > 0.0 and np.isfinite(out["refit_ms"])
    assert out["bad_vertices"] == 0
    assert out["tris_equal"] and out["nodes_equal"]


@pytest.mark.parametrize("width", [4, 8])
def test_many_refits_in_flight_fold_as_one_by_one(art, backend, options, width):
    """A host that refits every frame and never synchronises: every call folds the event pairs that have completed, and the figures
    and the tree come out as if each refit had been waited for."""
    _check_many_refits(_many_refits(art, backend, width))


MANY_SCRIPT = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import test_gpu_refit as T
be = art.Backend(devices=[0, 0])
out = {str(w): T._many_refits(art, be, w) for w in (4, 8)}
be.shutdown()
print("RESULT " + json.dumps(out))
'''


def test_many_refits_in_flight_on_two_contexts(art):
    """the same through the fan-out to a second context on the same GPU (a child process: the library is a process-wide singleton)"""
    r = subprocess.run([sys.executable, "-c", MANY_SCRIPT, art.ROOT], capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(line[0][7:])
    for w in ("4", "8"):
        _check_many_refits(out[w])


def test_refusals_and_bad_vertices(art, backend):
    from ada_ray_tracer_amd import scenes
    L = backend.lib
    backend.upload_scene(scenes.instanced_scene(n_instances=4, tris_per_mesh=200))
    with pytest.raises(art.ArtError, match="instanced"):
        backend.refit_torch(torch.zeros((10, 3), device="cuda"))
    backend.upload_scene(scenes.reference_scene())                      # the REFERENCE_BF pyramid only
    with pytest.raises(art.ArtError, match="no ART_MESH_CLOSEST"):
        backend.refit_torch(torch.zeros((10, 3), device="cuda"))
    sd = _scene("structured")
    pos, nrm, _, _ = _mesh(sd)
    backend.upload_scene(sd)
    n0, t0, _ = _export(backend)
    pg, ng = _gpu(pos, nrm)
    with pytest.raises(art.ArtError, match="nverts"):
        backend.refit_torch(pg[:-1])
    with pytest.raises(art.ArtError, match="GPU tensor"):
        backend.refit_torch(torch.from_numpy(pos))
    with pytest.raises(art.ArtError, match="shape"):
        backend.refit_torch(pg, ng[:-1])
    assert L.art_refit_device(C.c_void_p(pos.ctypes.data), None, len(pos), None) != 0           # host memory, straight through the C ABI
    assert "not device memory" in L.art_last_error().decode()
    assert L.art_refit_device(C.c_void_p(pg.data_ptr()), C.c_void_p(nrm.ctypes.data), len(pos), None) != 0
    assert "nrm3f" in L.art_last_error().decode()
    bad = pos.copy(); bad[5, 1] = np.nan; bad[9, 0] = np.inf; bad[11, 2] = F(3e18)
    with pytest.raises(ValueError, match="3 vertex"):
        backend.refit_torch(_gpu(bad)[0])
    assert backend.refit_info().refits == 0                                # nothing was launched
    n1, t1, _ = _export(backend)
    assert np.array_equal(n1, n0) and np.array_equal(t1, t0)

    p2, n2 = _deform("structured", pos, nrm)
    bad2 = p2.copy(); bad2[5, 1] = np.nan; bad2[9, 0] = np.inf; bad2[11, 2] = F(-3e18)
    backend.refit_torch(_gpu(bad2)[0], check=False)                       # returns; the boxes holding the bad vertices are emptied
    with pytest.raises(art.ArtError, match="3 vertex coordinate"):
        backend.synchronize()
    o, d = _rays(20000, 13)
    og, dg = _gpu(o, d)
    backend.trace_rays_torch(og, dg); backend.occluded_torch(og, dg)      # traversal of the emptied boxes ends
    backend.resize(32, 32)
    backend.render_pass(art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=3), 0)
    assert backend.refit_info().bad_vertices == 3
    _refit(backend, p2, n2)                                                # a good refit restores the state
    backend.synchronize()
    got = _observe(art, backend, o, d)
    backend.upload_scene(_moved(art, sd, p2, n2))
    _assert_same(got, _observe(art, backend, o, d))
