"""art_refit_mesh_device on the GPU: new vertices of ONE mesh of an instanced scene arrive in device memory, kernels rewrite the mesh's
records, refit its tree and bring pads, entry-point boxes and the instance tree up to date at the matrices in force, and the picture,
the ray count and the hit records are those of a fresh art_upload_scene of the scene with that mesh's vertices replaced (and
therefore the flattened scene's), bit for bit.  No tolerance anywhere."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

import conv
import hostsim
import orc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 0xADA5EED0 + 64           # scenes.instanced_scene's default: placement A; SEED + 1: B; SEED + 2: C
W, H = 96, 80


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mats(sd):
    return np.array([list(sd.desc.instances[i].m) for i in range(sd.desc.n_instances)], np.float32)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def placed(k, n=12, tris=300):
    from ada_ray_tracer_amd import scenes
    return scenes.instanced_scene(n, tris, seed=SEED + k)


def verts(sd, mesh):
    """(pos, nrm) of mesh number `mesh` of sd, float32 [nverts, 3]"""
    return sd._mesh_arrays[mesh][0].copy(), sd._mesh_arrays[mesh][1].copy()


def variant(art, sd, meshes=None, m=None):
    """A SceneDesc equal to sd but for the pos / nrm of the meshes in `meshes` ({mesh: (pos, nrm or None = sd's)}) and, with m, the matrices"""
    ms = []
    for k, (pos, nrm, idx, uv, matid) in enumerate(sd._mesh_arrays):
        p, n = (meshes or {}).get(k, (pos, nrm))
        ms.append(dict(mode=art.MESH_CLOSEST, pos=p, nrm=nrm if n is None else n, idx=idx, uv=uv, matid=matid))
    inst = [(int(sd.desc.instances[i].mesh), list(sd.desc.instances[i].m) if m is None else m[i]) for i in range(sd.desc.n_instances)]
    return art.SceneDesc(meshes=ms, instances=inst, **sd._kw)


def twisted(pos, nrm, sy=1.6, k=1.5):
    """rotation about y by k radians per unit of y, then y *= sy; the normals are turned along"""
    a = k * pos[:, 1].astype(np.float64)
    c, s = np.cos(a), np.sin(a)

    def rot(v):
        v = v.astype(np.float64)
        return np.stack([c * v[:, 0] + s * v[:, 2], v[:, 1], -s * v[:, 0] + c * v[:, 2]], 1)
    p = rot(pos); p[:, 1] *= sy
    n = rot(nrm); n[:, 1] /= sy; n /= np.linalg.norm(n, axis=1, keepdims=True)
    return p.astype(np.float32), n.astype(np.float32)


def mis(art):
    return art.Backend.pass_params(art.PT_MIS, True, 8, 2, seed=21)


def render(backend, p, w=W, h=H):
    backend.resize(w, h)
    accum, _, spp = backend.render_pass(p, 0)
    st = backend.stats()
    return accum.copy(), st.rays, st.lost_paths


def same(got, want):
    return got[1] == want[1] and got[2] == 0 and np.array_equal(bits(got[0]), bits(want[0]))


_fresh = {}


def fresh(art, backend, key, sd):
    """picture and ray count of a fresh upload of sd under the default options (computed once per key)"""
    if key not in _fresh:
        backend.upload_scene(sd)
        _fresh[key] = render(backend, mis(art))
    return _fresh[key]


def deformed_a(art):
    """placement A, its torus (mesh 0) twisted and stretched; and the new vertices"""
    A = placed(0)
    p, n = twisted(*verts(A, 0))
    return A, variant(art, A, {0: (p, n)}), p, n


@pytest.mark.parametrize("kernel", ["coop", "coop_stack_cap_3", "one_ray_per_lane"])
def test_a_mesh_refit_equals_a_fresh_upload_and_the_oracle_on_the_flattened_scene(art, backend, kernel):
    A, D, p, n = deformed_a(art)
    pp = mis(art)
    backend.set_option("inst_coop", 0 if kernel == "one_ray_per_lane" else 1)
    backend.set_option("lds_stack_cap", 3 if kernel == "coop_stack_cap_3" else 0)
    try:
        backend.upload_scene(D)
        want = render(backend, pp)
        backend.upload_scene(A)
        pic_a = render(backend, pp)
        backend.refit_mesh_torch(0, gpu(p), gpu(n))
        got = render(backend, pp)
    finally:
        backend.set_option("inst_coop", 1); backend.set_option("lds_stack_cap", 0)
    assert not np.array_equal(bits(pic_a[0]), bits(want[0]))              # (the deformation does something)
    assert want[2] == 0 and same(got, want)
    ref, _, cnt = orc.render(conv.OracleScene(hostsim.flattened_copy(art, D)).scene, orc.make_params(W, H, orc.PT_MIS, True, 8, 2, seed=21))
    assert got[1] == cnt.rays and np.array_equal(bits(got[0]), bits(ref))
    ri = backend.mesh_refit_info()
    assert ri.refits == 1 and ri.bad_vertices == 0 and ri.refit_ms > 0.0


@pytest.mark.parametrize("inst_open", [1, 8, 1000])
def test_opened_instances_follow_triangles_that_leave_their_entry_boxes(art, backend, inst_open):
    """stretched by 3 along x the torus' triangles lie well outside the boxes their entry points were opened with: stale entry boxes
    would leave holes"""
    A = placed(0)
    p, _ = verts(A, 0)
    p[:, 0] *= 3.0
    D = variant(art, A, {0: (p, None)})
    pp = mis(art)
    dbgp = art.Backend.pass_params(art.RT_DEBUG, False, 8, 1)
    backend.set_option("inst_open", inst_open)
    try:
        backend.upload_scene(D)
        want = render(backend, pp)
        want_dbg = backend.debug_hit_pass(dbgp)
        backend.upload_scene(A)
        backend.refit_mesh_torch(0, gpu(p))
        got = render(backend, pp)
        dbg = backend.debug_hit_pass(dbgp)
    finally:
        backend.set_option("inst_open", 0)
    assert same(got, want)
    assert np.array_equal(bits(dbg[0]), bits(want_dbg[0]))
    for k in (2, 3, 4):
        assert np.array_equal(dbg[k], want_dbg[k])
    assert (dbg[4] == 2).sum() > 300                                      # (the meshes are in the picture)


def test_normals_are_kept_or_replaced(art, backend):
    A, D, p, n = deformed_a(art)
    p0, n0 = verts(A, 0)
    pp = mis(art)
    pic_a = fresh(art, backend, "A", A)
    backend.upload_scene(variant(art, A, {0: (p, None)}))                 # new positions, old normals
    want_pos = render(backend, pp)
    backend.upload_scene(variant(art, A, {0: (p0, n)}))                   # old positions, new normals
    want_nrm = render(backend, pp)
    backend.upload_scene(A)
    backend.refit_mesh_torch(0, gpu(p), None)
    assert same(render(backend, pp), want_pos)
    backend.upload_scene(A)
    backend.refit_mesh_torch(0, gpu(p0), gpu(n))
    got = render(backend, pp)
    assert same(got, want_nrm) and not np.array_equal(bits(got[0]), bits(pic_a[0]))
    assert not np.array_equal(bits(want_pos[0]), bits(fresh(art, backend, "D", D)[0]))      # (the normals matter)


def _rays(n, seed):
    rng = np.random.default_rng(seed)
    o = (np.array([-2.4, 0.1, 0.1]) + rng.random((n, 3)) * np.array([4.8, 4.7, 4.7])).astype(np.float32)
    d = rng.normal(0.0, 1.0, (n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def test_both_meshes_and_back_reproduce_the_uploaded_trees(art, backend):
    """Deformations that stay inside the meshes' uploaded boxes ask for no wider pad, and an unmoved tree is reproduced bit for bit as
    long as no pad grew: after both meshes are back at the uploaded vertices the walk costs exactly what it cost after the upload.  A
    refit whose boxes only grow would pass every picture test and fail here."""
    A = placed(0)
    p0, n0 = verts(A, 0)
    p1, n1 = verts(A, 1)
    d0 = twisted(p0, n0, sy=0.7, k=1.2)                                   # (a rotation about y keeps the torus inside its box in x and z)
    d1 = ((p1 * np.array([0.9, 0.5, 0.9], np.float32)).astype(np.float32), n1)
    pp = mis(art)
    o, d = _rays(4096, 31)

    def walk():
        backend.set_option("count_tests", 1)
        try:
            hits, st = backend.trace_rays(o, d, want_stats=True)
        finally:
            backend.set_option("count_tests", 0)
        return bits([h.t for h in hits]), st.node_visits, st.box_tests
    backend.upload_scene(variant(art, A, {0: d0, 1: d1}))
    want_both = render(backend, pp)
    backend.upload_scene(A)
    want_a = render(backend, pp)
    t_a, nodes_a, boxes_a = walk()
    backend.refit_mesh_torch(1, gpu(d1[0]), gpu(d1[1]))
    backend.refit_mesh_torch(0, gpu(d0[0]), gpu(d0[1]))
    assert same(render(backend, pp), want_both)
    assert not np.array_equal(bits(want_both[0]), bits(want_a[0]))
    backend.refit_mesh_torch(0, gpu(p0), gpu(n0))
    backend.refit_mesh_torch(1, gpu(p1), gpu(n1))
    assert same(render(backend, pp), want_a)
    t, nodes, boxes = walk()
    ri = backend.mesh_refit_info()
    print("node_visits", nodes, nodes_a, "box_tests", boxes, boxes_a, "repads", ri.repads)
    assert ri.refits == 4 and ri.repads == 0 and ri.bad_vertices == 0
    assert np.array_equal(t, t_a) and nodes_a > 4096
    assert nodes == nodes_a and boxes == boxes_a


def test_interleaved_with_moves(art, backend):
    """the plan is shared with art_move_instances_device: whichever call comes first after the upload builds it, a move keeps the
    deformed mesh, a refit the matrices in force"""
    A, D, p, n = deformed_a(art)
    mB, mC = mats(placed(1)), mats(placed(2))
    pp = mis(art)
    want_b = fresh(art, backend, "D@B", variant(art, D, m=mB))
    want_c = fresh(art, backend, "D@C", variant(art, D, m=mC))
    assert not np.array_equal(bits(want_b[0]), bits(want_c[0]))
    backend.upload_scene(A)                                               # a move first
    backend.move_instances_torch(gpu(mB))
    backend.refit_mesh_torch(0, gpu(p), gpu(n))
    assert same(render(backend, pp), want_b)
    backend.move_instances_torch(gpu(mC))
    assert same(render(backend, pp), want_c)
    backend.upload_scene(A)                                               # a refit first
    backend.refit_mesh_torch(0, gpu(p), gpu(n))
    backend.move_instances_torch(gpu(mB))
    assert same(render(backend, pp), want_b)
    assert backend.mesh_refit_info().refits == 1 and backend.move_info().moves == 1


def speck_and_torus(art, grow=1.0):
    """scenes.speck_scene -- the bumpy grid (mesh 1) as a speck far from the origin, the camera right in front of it -- plus one instance of
    the torus (mesh 0) in the middle of the box, its vertices scaled by `grow`"""
    from ada_ray_tracer_amd import scenes
    speck = scenes.speck_scene()
    m = np.zeros((3, 4)); m[:, :3] = np.eye(3) * 0.3; m[:, 3] = (0.5, 2.0, 2.5)
    sd = scenes.instanced_scene(0, 600, transforms=[(1, np.array(list(speck.desc.instances[0].m)).reshape(3, 4)), (0, m)])
    cam = tuple(speck._kw["cam_pos"])
    for k in range(3):
        sd.desc.cam_pos[k] = cam[k]
    sd._kw["cam_pos"] = cam
    p, n = verts(sd, 0)
    return (sd if grow == 1.0 else variant(art, sd, {0: (p * np.float32(grow), None)})), p * np.float32(grow)


def test_a_mesh_that_grows_widens_the_other_meshes_pads(art, backend):
    """the torus at 40 times its size reaches 12 units out, past everything else in the scene: the extent E grows, and with it the pad the
    SPECK's boxes need (its inverse matrix is 2000: the ray taken to object space is that much further off)"""
    small, _ = speck_and_torus(art)
    big, p = speck_and_torus(art, 40.0)
    pp = art.Backend.pass_params(art.PT_MIS, True, 4, 1, seed=3)
    backend.upload_scene(big)
    want = render(backend, pp, 96, 96)
    backend.upload_scene(small)
    backend.refit_mesh_torch(0, gpu(p))
    got = render(backend, pp, 96, 96)
    ri = backend.mesh_refit_info()
    assert ri.repads >= 1 and backend.move_info().repads == 0
    assert want[2] == 0 and same(got, want) and (got[0] > 0).mean() > 0.5


def test_bad_vertices_are_counted_and_emptied(art, backend):
    A = placed(0)
    p0, n0 = verts(A, 0)
    bad = p0.copy()
    bad[3, 1] = np.nan
    bad[10, 0] = 1.0e19
    from ada_ray_tracer_amd import scenes
    want = fresh(art, backend, "A", A)
    dbgp = art.Backend.pass_params(art.RT_DEBUG, False, 8, 1)
    shift = int(np.ceil(np.log2(max(A.desc.meshes[k].ntris for k in range(2)))))
    mA = mats(A)
    without = scenes.instanced_scene(0, 300, transforms=[(1, mA[i].reshape(3, 4)) for i in range(12) if i % 2 == 1])      # the grid's instances alone
    backend.upload_scene(without); backend.resize(W, H)
    want_dbg = backend.debug_hit_pass(dbgp)
    backend.upload_scene(A); backend.resize(W, H)
    backend.refit_mesh_torch(0, gpu(bad), check=False)
    with pytest.raises(art.ArtError, match="art_refit_mesh_device: 2 vertex coordinate"):
        backend.synchronize()
    backend.synchronize()                                                 # reported once
    assert backend.mesh_refit_info().bad_vertices == 2
    # whole instances are the entry points here (instance k shows mesh k % 2), so every instance of the torus is empty and what is
    # left is the scene of the grid's instances alone: instance k of A is instance k // 2 of that scene
    dbg = backend.debug_hit_pass(dbgp)
    assert np.array_equal(bits(dbg[0]), bits(want_dbg[0])) and np.array_equal(dbg[3], want_dbg[3]) and np.array_equal(dbg[4], want_dbg[4])
    on = dbg[4] == 2
    assert on.any() and np.array_equal(dbg[2][~on], want_dbg[2][~on])
    inst = dbg[2][on] >> shift
    assert (inst % 2 == 1).all()
    assert np.array_equal(((inst >> 1) << shift) | (dbg[2][on] & ((1 << shift) - 1)), want_dbg[2][on])
    backend.refit_mesh_torch(0, gpu(p0))                                  # a good refit clears the state
    backend.synchronize()
    assert same(render(backend, mis(art)), want)
    with pytest.raises(ValueError, match="2 vertex position"):
        backend.refit_mesh_torch(0, gpu(bad))                             # check=True looks before anything is launched
    ri = backend.mesh_refit_info()
    assert ri.refits == 2 and ri.bad_vertices == 2


def test_a_good_refit_of_another_mesh_does_not_hide_a_mesh_that_is_still_bad(art, backend):
    A = placed(0)
    p0, _ = verts(A, 0)
    p1, _ = verts(A, 1)
    bad = p0.copy()
    bad[3, 1] = np.nan
    bad[10, 0] = 1.0e19
    want = fresh(art, backend, "A", A)
    backend.upload_scene(A)
    backend.refit_mesh_torch(0, gpu(bad), check=False)
    backend.refit_mesh_torch(1, gpu(p1), check=False)                     # good, and between the bad refit and the synchronize
    with pytest.raises(art.ArtError, match="art_refit_mesh_device: 2 vertex coordinate"):
        backend.synchronize()
    backend.synchronize()                                                 # reported once per refit
    backend.refit_mesh_torch(1, gpu(p1), check=False)                     # mesh 0 still holds its two
    with pytest.raises(art.ArtError, match="art_refit_mesh_device: 2 vertex coordinate"):
        backend.synchronize()
    bad1 = p1.copy()
    bad1[0, 2] = -np.inf
    backend.refit_mesh_torch(1, gpu(bad1), check=False)                   # the sum over the meshes
    with pytest.raises(art.ArtError, match="art_refit_mesh_device: 3 vertex coordinate"):
        backend.synchronize()
    backend.refit_mesh_torch(0, gpu(p0), check=False)                     # mesh 1's one is left
    with pytest.raises(art.ArtError, match="art_refit_mesh_device: 1 vertex coordinate"):
        backend.synchronize()
    backend.refit_mesh_torch(1, gpu(p1), check=False)
    backend.synchronize()
    assert same(render(backend, mis(art)), want)
    ri = backend.mesh_refit_info()
    assert ri.refits == 6 and ri.bad_vertices == 3                        # (cumulative: 2 + 1)


def test_stream_order(art, backend):
    A, D, p, n = deformed_a(art)
    o, d = _rays(4096, 17)
    o, d = gpu(o), gpu(d)
    backend.upload_scene(D)
    want_d = backend.trace_rays_torch(o, d).raw.cpu().numpy()
    backend.upload_scene(A)
    want_a = backend.trace_rays_torch(o, d).raw.cpu().numpy()
    assert not np.array_equal(want_a, want_d)
    gp, gn = gpu(p), gpu(n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h1 = backend.trace_rays_torch(o, d)
        backend.refit_mesh_torch(0, gp, gn, check=False)                  # (check=False: no host synchronisation in between)
        h2 = backend.trace_rays_torch(o, d)
    s.synchronize()
    assert np.array_equal(h1.raw.cpu().numpy(), want_a)
    assert np.array_equal(h2.raw.cpu().numpy(), want_d)
    assert np.array_equal(backend.trace_rays_torch(o, d).raw.cpu().numpy(), want_d)


def test_refusals(art, backend):
    from ada_ray_tracer_amd import scenes
    L = backend.lib
    pp = mis(art)
    A = placed(0)
    p0, _ = verts(A, 0)
    backend.upload_scene(scenes.synthetic_scene(2000, 3))
    want = render(backend, pp)
    with pytest.raises(art.ArtError, match="not instanced.*art_refit_device"):
        backend.refit_mesh_torch(0, gpu(p0))
    assert same(render(backend, pp), want)
    speck = scenes.speck_scene()                                          # (shows its grid only)
    backend.upload_scene(speck)
    with pytest.raises(art.ArtError, match="no instance shows mesh 0"):
        backend.refit_mesh_torch(0, gpu(verts(speck, 0)[0]))
    backend.upload_scene(A)
    want = fresh(art, backend, "A", A)
    backend.upload_scene(A)
    g = gpu(p0)
    for mesh in (-1, 2):
        with pytest.raises(art.ArtError, match="mesh %d is out of range" % mesh):
            backend.refit_mesh_torch(mesh, g)
    for q in (p0[:-1], np.concatenate([p0, p0[:1]])):
        with pytest.raises(art.ArtError, match="nverts"):
            backend.refit_mesh_torch(0, gpu(q))
    with pytest.raises(art.ArtError, match="nverts"):
        backend.refit_mesh_torch(1, g)                                    # the other mesh's count
    with pytest.raises(art.ArtError, match="GPU tensor"):
        backend.refit_mesh_torch(0, torch.from_numpy(p0))
    n = p0.shape[0]
    assert L.art_refit_mesh_device(0, C.c_void_p(p0.ctypes.data), None, n, None) != 0      # host memory, straight through the C ABI
    assert "pos3f is not device memory" in L.art_last_error().decode()
    assert L.art_refit_mesh_device(0, g.data_ptr(), C.c_void_p(p0.ctypes.data), n, None) != 0
    assert "nrm3f is not device memory" in L.art_last_error().decode()
    assert L.art_refit_mesh_device(0, None, None, n, None) != 0
    assert "null pos3f" in L.art_last_error().decode()
    assert backend.mesh_refit_info().refits == 0                          # nothing was launched
    assert same(render(backend, pp), want)


SCRIPT = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import torch
import ctypes as C
import test_gpu_refit_mesh as T
out = {}
A, D, p, n = T.deformed_a(art)
pp = T.mis(art)
be = art.Backend(0)
L = be.lib
try:
    be.refit_mesh_torch(0, T.gpu(p))
    out["no_scene"] = "accepted"
except art.ArtError as e:
    out["no_scene"] = str(e)
verts = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0); tri = (C.c_int * 3)(0, 1, 2)
L.gcore_init_and_clear()
L.gcore_instance_meshes(L.gcore_add_mesh_3f(verts, 3, tri, 3), (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1), 1)
L.gcore_commit_scene()
o = (C.c_float * 3)(0.25, 0.25, 1.0); d = (C.c_float * 3)(0.0, 0.0, -1.0)
h0 = art.HitCpp(); hit0 = bool(L.gcore_closest_hit(o, d, 0.0, 100.0, C.byref(h0)))
try:
    be.refit_mesh_torch(0, torch.zeros((3, 3), device="cuda"))
    out["gcore"] = "accepted"
except art.ArtError as e:
    out["gcore"] = str(e)
h1 = art.HitCpp(); hit1 = bool(L.gcore_closest_hit(o, d, 0.0, 100.0, C.byref(h1)))
out["gcore_unchanged"] = bool(hit0 == hit1 and h0.t == h1.t and h0.primIndex == h1.primIndex)
L.gcore_destroy()
be.upload_scene(D)
ref = T.render(be, pp)
be.shutdown()
be = art.Backend(devices=[0, 0])
be.upload_scene(A)
T.render(be, pp)                                             # (the old shape rendered once on every context)
be.refit_mesh_torch(0, T.gpu(p), T.gpu(n))
got = T.render(be, pp)
out["two_contexts"] = bool(T.same(got, ref))
out["refits"] = be.mesh_refit_info().refits
be.shutdown()
print("RESULT " + json.dumps(out))
'''


def test_two_contexts_on_one_gpu_and_the_refusals_of_a_fresh_process(art):
    """art_init_devices([0, 0]) in a child process (the library is a process-wide singleton): every context is refitted, the second from
    a peer copy of the vertices; and the refusals that need a fresh process: no scene, a scene committed through the gcore seam"""
    r = subprocess.run([sys.executable, "-c", SCRIPT, art.ROOT], capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(line[0][7:])
    assert "art_refit_mesh_device: no scene uploaded" in out["no_scene"]
    assert "gcore_commit_scene" in out["gcore"] and out["gcore_unchanged"]
    assert out["two_contexts"] and out["refits"] == 1
