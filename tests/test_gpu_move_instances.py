"""art_move_instances_device on the GPU: new instance matrices arrive in device memory, kernels bring the instance table, the entry
points' boxes, the instance tree and -- where the new placement outgrows them -- the pads of the meshes' boxes up to date, and the
picture, the ray count and the hit records are those of a fresh art_upload_scene at the new matrices (and therefore the flattened
scene's), bit for bit.  No tolerance anywhere."""
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


def gpu(m):
    return torch.from_numpy(np.ascontiguousarray(m, np.float32)).cuda()


def placed(k, n=12, tris=300):
    from ada_ray_tracer_amd import scenes
    return scenes.instanced_scene(n, tris, seed=SEED + k)


def with_mats(sd, m, **kw):
    """sd's meshes and mesh-per-instance under the matrices m"""
    from ada_ray_tracer_amd import scenes
    tris = kw.pop("tris", 300)
    return scenes.instanced_scene(0, tris, transforms=[(int(sd.desc.instances[i].mesh), m[i].reshape(3, 4)) for i in range(len(m))], **kw)


def mis(art):
    return art.Backend.pass_params(art.PT_MIS, True, 8, 2, seed=21)


def render(backend, p, w=W, h=H):
    backend.resize(w, h)
    accum, _, spp = backend.render_pass(p, 0)
    st = backend.stats()
    return accum.copy(), st.rays, st.lost_paths


_fresh = {}


def fresh(art, backend, key, sd):
    """picture and ray count of a fresh upload of sd under the default options (computed once per key)"""
    if key not in _fresh:
        backend.upload_scene(sd)
        _fresh[key] = render(backend, mis(art))
    return _fresh[key]


@pytest.mark.parametrize("kernel", ["coop", "coop_stack_cap_3", "one_ray_per_lane"])
def test_a_move_equals_a_fresh_upload_and_the_oracle_on_the_flattened_scene(art, backend, kernel):
    A, B = placed(0), placed(1)
    p = mis(art)
    backend.set_option("inst_coop", 0 if kernel == "one_ray_per_lane" else 1)
    backend.set_option("lds_stack_cap", 3 if kernel == "coop_stack_cap_3" else 0)
    try:
        backend.upload_scene(B)
        want, want_rays, _ = render(backend, p)
        backend.upload_scene(A)
        pic_a, _, _ = render(backend, p)
        backend.move_instances_torch(gpu(mats(B)).reshape(12, 3, 4))
        got, rays, lost = render(backend, p)
    finally:
        backend.set_option("inst_coop", 1); backend.set_option("lds_stack_cap", 0)
    assert not np.array_equal(bits(pic_a), bits(want))                    # (the move does something)
    assert rays == want_rays and lost == 0
    assert np.array_equal(bits(got), bits(want))
    ref, _, cnt = orc.render(conv.OracleScene(hostsim.flattened_copy(art, B)).scene, orc.make_params(W, H, orc.PT_MIS, True, 8, 2, seed=21))
    assert rays == cnt.rays and np.array_equal(bits(got), bits(ref))
    mi = backend.move_info()
    assert mi.moves == 1 and mi.bad_matrices == 0 and mi.move_ms > 0.0


@pytest.mark.parametrize("inst_open", [1, 8, 1000])
def test_a_move_to_mirrored_sheared_coincident_tiny_and_huge_instances(art, backend, inst_open):
    """the instance tree is built (and opened) for ordinary matrices, then the instances move to hostsim.awkward_instances: the 1e-3
    instance asks for a thousand times the pad its mesh's boxes were built with"""
    from ada_ray_tracer_amd import scenes
    tr = hostsim.awkward_instances()
    n = len(tr)
    target = scenes.instanced_scene(0, 260, transforms=tr, all_materials=True)
    start = with_mats(target, mats(placed(0, n)), tris=260, all_materials=True)
    flat = hostsim.flattened_copy(art, target)
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 2, seed=77)
    dbgp = art.Backend.pass_params(art.RT_DEBUG, False, 8, 1)
    backend.set_option("inst_open", inst_open)
    try:
        backend.upload_scene(target)
        want, want_rays, _ = render(backend, p, 128, 96)
        want_dbg = backend.debug_hit_pass(dbgp)
        backend.upload_scene(start)
        backend.move_instances_torch(gpu(mats(target)))
        got, rays, lost = render(backend, p, 128, 96)
        dbg = backend.debug_hit_pass(dbgp)
        repads = backend.move_info().repads
    finally:
        backend.set_option("inst_open", 0)
    assert rays == want_rays and lost == 0 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(dbg[0]), bits(want_dbg[0]))
    for k in (2, 3, 4):
        assert np.array_equal(dbg[k], want_dbg[k])
    assert repads >= 1
    backend.upload_scene(flat); backend.resize(128, 96)
    ref_dbg = backend.debug_hit_pass(dbgp)
    ntris = [target.desc.meshes[mi].ntris for mi, _ in tr]
    offs = np.concatenate([[0], np.cumsum(ntris)])
    shift = int(np.ceil(np.log2(max(ntris))))
    prim, ptype, rprim = dbg[2], dbg[4], ref_dbg[2]
    assert np.array_equal(bits(dbg[0]), bits(ref_dbg[0])) and np.array_equal(dbg[3], ref_dbg[3]) and np.array_equal(ptype, ref_dbg[4])
    on_mesh = (ptype == 2)
    assert np.array_equal(prim[~on_mesh], rprim[~on_mesh]) and on_mesh.sum() > 500
    inst = prim[on_mesh] >> shift
    assert np.array_equal(offs[inst] + (prim[on_mesh] & ((1 << shift) - 1)), rprim[on_mesh])


@pytest.mark.parametrize("view", [(2.0, 1.0), (1.5, 0.1)])
def test_a_move_to_the_speck_widens_the_pads(art, backend, view):
    """uploaded at scale 0.3 the grid's boxes carry the floor pad; moved to scale 5e-4 far from the origin they need the speck's, or the
    object-space box test culls triangles the world-space test accepts (tests/test_instanced_host_sim.py test_a_speck_far_from_the_origin)"""
    from ada_ray_tracer_amd import scenes
    speck = scenes.speck_scene(view=view)
    big = scenes.speck_scene(view=view)
    for k in (0, 5, 10):
        big.desc.instances[0].m[k] = 0.3
    p = art.Backend.pass_params(art.PT_MIS, True, 4, 1, seed=3)
    backend.upload_scene(hostsim.flattened_copy(art, speck))
    want, want_rays, _ = render(backend, p, 96, 96)
    backend.upload_scene(big)
    backend.move_instances_torch(gpu(mats(speck)))
    got, rays, lost = render(backend, p, 96, 96)
    assert backend.move_info().repads >= 1
    assert rays == want_rays and lost == 0 and (got > 0).mean() > 0.5
    assert np.array_equal(bits(got), bits(want))


def test_sequences_of_moves(art, backend):
    A, B, Cc = placed(0), placed(1), placed(2)
    p = mis(art)
    pa, pb, pc = fresh(art, backend, "A", A), fresh(art, backend, "B", B), fresh(art, backend, "C", Cc)
    backend.upload_scene(A)
    backend.move_instances_torch(gpu(mats(A)))                            # a move to where they are
    got = render(backend, p)
    assert got[1] == pa[1] and got[2] == 0 and np.array_equal(bits(got[0]), bits(pa[0]))
    backend.move_instances_torch(gpu(mats(B)))
    backend.move_instances_torch(gpu(mats(Cc)))
    got = render(backend, p)
    assert got[1] == pc[1] and got[2] == 0 and np.array_equal(bits(got[0]), bits(pc[0]))
    backend.move_instances_torch(gpu(mats(B)))
    backend.move_instances_torch(gpu(mats(A)))                            # back home: the pads may have grown, the picture must not care
    got = render(backend, p)
    assert got[1] == pa[1] and got[2] == 0 and np.array_equal(bits(got[0]), bits(pa[0]))
    assert backend.move_info().moves == 5
    assert not np.array_equal(bits(pa[0]), bits(pb[0])) and not np.array_equal(bits(pb[0]), bits(pc[0]))


def test_instances_that_swap_places(art, backend):
    """the translations permuted among the instances: every instance tree leaf now bounds something far from its neighbours"""
    A, B = placed(0), placed(1)
    m = mats(B).reshape(12, 3, 4).copy()
    m[:, :, 3] = np.roll(m[:, :, 3], 5, axis=0)
    Bp = with_mats(B, m.reshape(12, 12))
    p = mis(art)
    backend.upload_scene(Bp)
    want = render(backend, p)
    backend.upload_scene(A)
    backend.move_instances_torch(gpu(m))
    got = render(backend, p)
    assert got[1] == want[1] and got[2] == 0 and np.array_equal(bits(got[0]), bits(want[0]))
    assert not np.array_equal(bits(want[0]), bits(fresh(art, backend, "B", B)[0]))


def _rays(n, seed):
    rng = np.random.default_rng(seed)
    o = (np.array([-2.4, 0.1, 0.1]) + rng.random((n, 3)) * np.array([4.8, 4.7, 4.7])).astype(np.float32)
    d = rng.normal(0.0, 1.0, (n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return gpu(o), gpu(d)


def test_queries_after_a_move_and_stream_order(art, backend):
    A, B = placed(0), placed(1)
    o, d = _rays(4096, 17)
    kernels = (art.TRACE_COOP, art.TRACE_SIMPLE)

    def ask():
        return [backend.trace_rays_torch(o, d, kernel=k).raw.cpu().numpy() for k in kernels] + [backend.occluded_torch(o, d).cpu().numpy()]
    backend.upload_scene(B)
    want_b = ask()
    backend.upload_scene(A)
    want_a = ask()
    assert not np.array_equal(want_a[0], want_b[0]) and want_b[2].any() and not want_b[2].all()
    mb = gpu(mats(B))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h1 = backend.trace_rays_torch(o, d)
        backend.move_instances_torch(mb, check=False)                     # (check=False: no host synchronisation in between)
        h2 = backend.trace_rays_torch(o, d)
    s.synchronize()
    assert np.array_equal(h1.raw.cpu().numpy(), want_a[0])
    assert np.array_equal(h2.raw.cpu().numpy(), want_b[0])
    got = ask()
    for g, w in zip(got, want_b):
        assert np.array_equal(g, w)


def test_host_pointer_queries_after_a_move(art, backend):
    """art_trace_rays takes the shading normal of a mesh hit from the HOST copy of the instance table (the inverse matrices): after a
    move it must be the moved table's"""
    A, B = placed(0), placed(1)
    o, d = _rays(4096, 23)
    o, d = o.cpu().numpy(), d.cpu().numpy()

    def rows(h):
        return np.array([[x.is_hit, x.prim_type, x.prim_index, x.mat_id, x.mat] for x in h], np.int64), bits([[x.t, x.u, x.v] + list(x.normal) for x in h])
    backend.upload_scene(B)
    want = rows(backend.trace_rays(o, d))
    backend.upload_scene(A)
    old = rows(backend.trace_rays(o, d))
    backend.move_instances_torch(gpu(mats(B)))
    got = rows(backend.trace_rays(o, d))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    mesh = (want[0][:, 0] == 1) & (want[0][:, 1] == 2)
    assert mesh.sum() > 50 and not np.array_equal(old[1][mesh, 3:], want[1][mesh, 3:])       # (mesh hits exist -- 12 instances of about 0.5 m2 in a 106 m3 box: some 15 % of the rays -- and their normals did move)


@pytest.mark.parametrize("how", ["nan", "zeros"])
def test_a_bad_matrix_empties_its_instance(art, backend, how):
    A, B = placed(0), placed(1)
    dbgp = art.Backend.pass_params(art.RT_DEBUG, False, 8, 1)
    shift = int(np.ceil(np.log2(max(B.desc.meshes[k].ntris for k in range(2)))))
    backend.upload_scene(B); backend.resize(W, H)
    full = backend.debug_hit_pass(dbgp)
    on = full[4] == 2
    k = int(np.bincount(full[2][on] >> shift, minlength=12).argmax())      # the instance most pixels see
    mB = mats(B)
    from ada_ray_tracer_amd import scenes
    without = scenes.instanced_scene(0, 300, transforms=[(int(B.desc.instances[i].mesh), mB[i].reshape(3, 4)) for i in range(12) if i != k])
    ref = fresh(art, backend, "B", B)
    backend.upload_scene(without); backend.resize(W, H)
    want = backend.debug_hit_pass(dbgp)
    bad = mB.copy()
    bad[k] = 0.0
    if how == "nan":
        bad[k, 6] = np.nan
    backend.upload_scene(A); backend.resize(W, H)
    for count in (1, 2):
        backend.move_instances_torch(gpu(bad), check=False)
        with pytest.raises(art.ArtError, match="1 instance matrix"):
            backend.synchronize()
        backend.synchronize()                                             # reported once
        got = backend.debug_hit_pass(dbgp)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
        on = got[4] == 2
        assert np.array_equal(got[2][~on], want[2][~on])
        inst = got[2][on] >> shift
        assert not (inst == k).any()
        assert np.array_equal(((inst - (inst > k)) << shift) | (got[2][on] & ((1 << shift) - 1)), want[2][on])
        assert backend.move_info().bad_matrices == count
        backend.move_instances_torch(gpu(mB))                             # a good move clears the state
        backend.synchronize()
        pic = render(backend, mis(art))
        assert pic[1] == ref[1] and pic[2] == 0 and np.array_equal(bits(pic[0]), bits(ref[0]))
        backend.resize(W, H)
    if how == "nan":
        with pytest.raises(ValueError, match="1 matrix"):
            backend.move_instances_torch(gpu(bad))                        # check=True looks before anything is launched


def test_refusals(art, backend):
    from ada_ray_tracer_amd import scenes
    L = backend.lib
    p = mis(art)
    flat = scenes.synthetic_scene(2000, 3)
    backend.upload_scene(flat)
    want = render(backend, p)
    with pytest.raises(art.ArtError, match="not instanced"):
        backend.move_instances_torch(torch.zeros((12, 3, 4), device="cuda"))
    got = render(backend, p)
    assert got[1] == want[1] and np.array_equal(bits(got[0]), bits(want[0]))
    A = placed(0)
    backend.upload_scene(A)
    want = render(backend, p)
    mB = mats(placed(1))
    for m in (mB[:-1], np.concatenate([mB, mB[:1]])):
        with pytest.raises(art.ArtError, match="n_instances"):
            backend.move_instances_torch(gpu(m))
    with pytest.raises(art.ArtError, match="GPU tensor"):
        backend.move_instances_torch(torch.from_numpy(mB))
    assert L.art_move_instances_device(C.c_void_p(mB.ctypes.data), 12, None) != 0       # host memory, straight through the C ABI
    assert "not device memory" in L.art_last_error().decode()
    assert L.art_move_instances_device(None, 12, None) != 0
    assert "null m12f" in L.art_last_error().decode()
    assert backend.move_info().moves == 0                                  # nothing was launched
    got = render(backend, p)
    assert got[1] == want[1] and np.array_equal(bits(got[0]), bits(want[0]))


def _many_moves(art, be, n=200):
    """Placement A uploaded, then n moves back to back on a side stream with nothing waited for in between -- alternately to A's and to
    B's matrices, the last one to B's -- and ONE synchronize.  Returns ArtMoveInfo's figures and the picture."""
    A, B = placed(0), placed(1)
    be.upload_scene(A)
    g = [gpu(mats(A)), gpu(mats(B))]
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        for k in range(n):
            be.move_instances_torch(g[k % 2], check=False)
    be.synchronize()
    mi = be.move_info()
    return dict(moves=int(mi.moves), move_ms=float(mi.move_ms), bad_matrices=int(mi.bad_matrices)), render(be, mis(art))


def _check_many_moves(info, same, n=200):
    print("many moves:", info)
    assert info["moves"] == n
    assert info["move_ms"] > 0.0 and np.isfinite(info["move_ms"]) and info["bad_matrices"] == 0
    assert same


def test_many_moves_in_flight(art, backend):
    """A host that moves every frame and never synchronises: the figures and the picture come out as if each move had been waited for."""
    want = fresh(art, backend, "B", placed(1))
    info, got = _many_moves(art, backend)
    _check_many_moves(info, got[1] == want[1] and got[2] == 0 and np.array_equal(bits(got[0]), bits(want[0])))


MANY_SCRIPT = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import test_gpu_move_instances as T
be = art.Backend(0)
be.upload_scene(T.placed(1))
want = T.render(be, T.mis(art))
be.shutdown()
be = art.Backend(devices=[0, 0])
info, got = T._many_moves(art, be)
be.shutdown()
same = bool(got[1] == want[1] and got[2] == 0 and np.array_equal(T.bits(got[0]), T.bits(want[0])))
print("RESULT " + json.dumps(dict(info=info, same=same)))
'''


def test_many_moves_in_flight_on_two_contexts(art):
    """the same through the fan-out to a second context on the same GPU (a child process: the library is a process-wide singleton)"""
    r = subprocess.run([sys.executable, "-c", MANY_SCRIPT, art.ROOT], capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(line[0][7:])
    _check_many_moves(out["info"], out["same"])


SCRIPT = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import torch
import ctypes as C
import test_gpu_move_instances as T
out = {}
A, B = T.placed(0), T.placed(1)
p = T.mis(art)
be = art.Backend(0)
L = be.lib
verts = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0); tri = (C.c_int * 3)(0, 1, 2)
L.gcore_init_and_clear()
L.gcore_instance_meshes(L.gcore_add_mesh_3f(verts, 3, tri, 3), (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1), 1)
L.gcore_commit_scene()
o = (C.c_float * 3)(0.25, 0.25, 1.0); d = (C.c_float * 3)(0.0, 0.0, -1.0)
h0 = art.HitCpp(); hit0 = bool(L.gcore_closest_hit(o, d, 0.0, 100.0, C.byref(h0)))
try:
    be.move_instances_torch(torch.zeros((1, 3, 4), device="cuda"))
    out["gcore"] = "accepted"
except art.ArtError as e:
    out["gcore"] = str(e)
h1 = art.HitCpp(); hit1 = bool(L.gcore_closest_hit(o, d, 0.0, 100.0, C.byref(h1)))
out["gcore_unchanged"] = bool(hit0 == hit1 and h0.t == h1.t and h0.primIndex == h1.primIndex)
L.gcore_destroy()
be.upload_scene(B)
ref = T.render(be, p)
be.shutdown()
be = art.Backend(devices=[0, 0])
be.upload_scene(A)
T.render(be, p)                                              # (the old placement rendered once on every context)
be.move_instances_torch(T.gpu(T.mats(B)))
got = T.render(be, p)
out["two_contexts"] = bool(np.array_equal(T.bits(got[0]), T.bits(ref[0])) and got[1] == ref[1] and got[2] == 0)
out["moves"] = be.move_info().moves
be.shutdown()
print("RESULT " + json.dumps(out))
'''


def test_two_contexts_on_one_gpu_and_the_gcore_refusal(art):
    """art_init_devices([0, 0]) in a child process (the library is a process-wide singleton): every context is moved, the second from a
    peer copy of the matrices; and the refusal that needs a fresh process, a scene committed through the gcore seam"""
    r = subprocess.run([sys.executable, "-c", SCRIPT, art.ROOT], capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(line[0][7:])
    assert "gcore_commit_scene" in out["gcore"] and out["gcore_unchanged"]
    assert out["two_contexts"] and out["moves"] == 1
