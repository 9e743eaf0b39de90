"""art_rebuild_mesh_tree_device on the GPU: after a mesh refit the tree of that one mesh is built again from its records in HBM.
With whole instances the two-level scene after refit + mesh rebuild + instance-tree rebuild is the fresh upload's of the deformed
scene, word for word; the meshes behind the rebuilt one move and every word that names their nodes moves with them; nothing visible
changes; later updates work against the new layout; the cost figure is numpy's.  The yardstick is export_two_level(); every
comparison but the cost figure's (1e-9, tests/test_gpu_rebuild.py's bound) is exact."""
import json
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import hostsim
import two_level_ref as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 64
# The deformation: every coordinate warped inside the mesh's own box (u -> u ^ g per axis), so the box, the scene's extent and with them
# the mesh's pad keep their bits.  Node counts of the two prototype meshes by hostsim.two_level: (torus 15, grid 5) as uploaded,
# torus 16 with the torus warped, grid 3 with the grid warped -- asserted where the pairs are used.
WARP = (2.0, 1.0, 0.5)
STRONG = (6.0, 6.0, 6.0)


def R():
    import test_gpu_two_level_reference as mod
    return mod


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).cuda()


def warp(p, g=WARP):
    lo, hi = p.min(0), p.max(0)
    return (lo + (hi - lo) * ((p - lo) / (hi - lo)) ** np.asarray(g, F)).astype(F)


def deformed(art, sd, m, g=WARP):
    """(sd with mesh m warped, the warped positions)"""
    q = warp(R().verts(sd, m)[0], g)
    return R().variant(art, sd, {m: (q, None)}), q


@pytest.fixture
def options(backend):
    yield backend.set_option
    for name, v in (("inst_open", 0), ("inst_coop", 1), ("lds_stack_cap", 0)):
        backend.set_option(name, v)


_host = {}


def host_build(art, key, sd, inst_open=1):
    """hostsim.two_level of sd (computed once per key and left unchanged)"""
    if key not in _host:
        hostsim.set_bvh_param(art, "inst_open", inst_open)
        try:
            _host[key] = hostsim.two_level(art, sd)
        finally:
            hostsim.set_bvh_param(art, "inst_open", 0)
    return _host[key]


def nodes_of(ex, m):
    return ref.mesh_slices(ex, m)[1]


def assert_same(got, want, what):
    assert got["n_inst"] == want["n_inst"], what
    for name in ref.ARRAYS:
        assert got[name].shape == want[name].shape, "%s: shape of %s: %r, %r" % (what, name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), "%s: %s" % (what, name)


def distinct_centroids(sd, m, pos):
    c = np.asarray(pos, F)[R().verts(sd, m)[2]].mean(1)
    return len(np.unique(c, axis=0)) == len(c)


def walk_all(ex):
    """the merged array walked as the cooperative kernel does: the instance tree (test_gpu_rebuild_instances.walk), then every mesh
    from its root: every node of every mesh reached exactly once and only from its own mesh, every leaf inside its mesh's records,
    every entry point inside its own mesh's tree and where its root_entry says"""
    from test_gpu_rebuild_instances import walk
    n_tlas, n_entry = ex["tlas_nodes"].shape[0], ex["inst"].shape[0]
    assert sorted(walk(ex)) == list(range(n_entry))
    q = ex["qnodes"]
    nm = ex["mesh_base"].shape[0]
    seen = np.zeros(q.shape[0], bool)
    for m in range(nm):
        nb, nn, tb, nt, qb = ref.mesh_slices(ex, m)
        assert qb == n_tlas + nb
        todo = [qb]
        while todo:
            n = todo.pop()
            assert qb <= n < qb + nn and not seen[n], "mesh %d node %d" % (m, n)
            seen[n] = True
            assert ex["node_mesh"][n - n_tlas] == m
            for j in range(4):
                e = int(q[n, 4 * j + 2])
                r_, c_ = int(ex["blas_nodes"][n - n_tlas, 4 * j + 3:4 * j + 4].view(np.int32)[0]), int(ex["blas_nodes"][n - n_tlas, 19 + 4 * j:20 + 4 * j].view(np.int32)[0])
                if e == 0x80000000:
                    assert r_ < 0
                elif e & 0x80000000:
                    first, cnt = (e & 0x7FFFFFF0) // 64, e & 15
                    assert 1 <= cnt <= 4 and cnt == c_
                    if tb >= 0:                                           # (tb < 0: a mesh no instance shows, whose records the plan does not place)
                        assert first == tb + r_ and tb <= first and first + cnt <= tb + nt
                else:
                    assert e % 64 == 0 and c_ == 0 and e // 64 == qb + r_
                    todo.append(e // 64)
    assert seen[n_tlas:].all()
    inst = ex["inst"]
    for e in range(n_entry):
        node_base, tri_base = int(inst[e, ref.NODE_BASE].view(np.int32)), int(inst[e, ref.TRI_BASE].view(np.int32))
        root, qroot = int(inst[e, ref.ROOT_ENTRY].view(np.int32)), int(inst[e, ref.QROOT])
        m = [k for k in range(nm) if int(ex["mesh_base"][k, 1]) == tri_base][0]
        nb, nn, tb, nt, qb = ref.mesh_slices(ex, m)
        assert node_base == nb
        if root & 15:
            assert qroot == (0x80000000 | ((tb + (root >> 4)) * 64) | (root & 15))
        else:
            assert (root >> 4) < nn and qroot == (qb + (root >> 4)) * 64


# ---- 1. the tree is the upload's ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 12])
@pytest.mark.parametrize("m", [0, 1])
@pytest.mark.parametrize("direction", ["A_to_B", "B_to_A"])
def test_refit_rebuild_mesh_rebuild_instances_equals_a_fresh_upload(art, backend, options, n, m, direction):
    A = R().placed(0, n)
    B, qB = deformed(art, A, m)
    hostA, hostB = host_build(art, ("A", n), A), host_build(art, ("B", n, m), B)
    assert nodes_of(hostA, m) != nodes_of(hostB, m)                         # (i) picked on the CPU: the node count changes
    assert np.array_equal(bits(hostA["mesh_pad"]), bits(hostB["mesh_pad"]))     # (ii) the pads keep their bits
    assert distinct_centroids(A, m, R().verts(A, m)[0]) and distinct_centroids(A, m, qB)      # (iii) no ties between the builders' rules
    src, dst, pos = (A, B, qB) if direction == "A_to_B" else (B, A, R().verts(A, m)[0])
    options("inst_open", 1)
    backend.upload_scene(dst)
    fresh = backend.export_two_level()
    backend.upload_scene(src)
    before = backend.export_two_level()
    backend.refit_mesh_torch(m, gpu(pos))
    backend.rebuild_mesh(m)
    mid = backend.export_two_level()
    backend.rebuild_instances()
    got = backend.export_two_level()
    assert got["updated"] == 1
    assert_same(got, fresh, "against a fresh upload")
    assert_same(got, host_build(art, ("A", n), A) if dst is A else hostB, "against the host build")
    assert nodes_of(got, m) != nodes_of(before, m)
    # the mesh rebuild itself left the instance tree alone, and the other mesh's packets and records as they were
    for name in ("tlas_nodes", "tlas_tris"):
        assert np.array_equal(bits(mid[name]), bits(ref.refit_mesh(before, m, R().verts(A, m)[2], pos)[name])), name
    o = 1 - m
    nb0, nn0, tb0, nt0, _ = ref.mesh_slices(before, o)
    nb1, nn1, tb1, nt1, _ = ref.mesh_slices(mid, o)
    assert nn0 == nn1 and (tb0, nt0) == (tb1, nt1) and (nb1 != nb0) == (m == 0)      # (the mesh behind the rebuilt one relocates)
    assert np.array_equal(bits(mid["blas_nodes"][nb1:nb1 + nn1]), bits(before["blas_nodes"][nb0:nb0 + nn0]))
    assert np.array_equal(bits(mid["blas_tris"][tb1:tb1 + nt1]), bits(before["blas_tris"][tb0:tb0 + nt0]))
    walk_all(mid)
    ri = backend.mesh_rebuild_info()
    assert ri.rebuilds == 1 and ri.gather_ms > 0.0 and ri.build_ms > 0.0 and ri.host_ms >= ri.build_ms


# ---- 2. nothing visible changes ---------------------------------------------------------------------------------------------------------
def _rays(n=4096, seed=11):
    rng = np.random.default_rng(seed)
    o = np.stack([-2.4 + 4.8 * rng.random(n), 0.2 + 4.4 * rng.random(n), 0.2 + 4.6 * rng.random(n)], 1).astype(F)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return gpu(o), gpu(d)


def _visible(art, backend):
    backend.resize(W, H)
    accum, _, spp = backend.render_pass(art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=7), 0)
    assert spp == 4
    st = backend.stats()
    o, d = _rays()
    hits = backend.trace_rays_torch(o, d).raw.cpu().numpy()
    assert st.lost_paths == 0
    return bits(accum).copy(), int(st.rays), hits


@pytest.mark.parametrize("kernel", ["coop", "coop_stack_cap_5", "one_ray_per_lane"])
def test_picture_hits_and_ray_count_do_not_change(art, backend, options, kernel):
    A = R().placed(0, 12)
    B, qB = deformed(art, A, 0)
    options("inst_coop", 0 if kernel == "one_ray_per_lane" else 1)
    options("lds_stack_cap", 5 if kernel == "coop_stack_cap_5" else 0)
    backend.upload_scene(hostsim.flattened_copy(art, B))
    flat_picture = _visible(art, backend)[0]
    backend.upload_scene(A)
    backend.refit_mesh_torch(0, gpu(qB))
    refitted = _visible(art, backend)
    n_before = nodes_of(backend.export_two_level(), 0)
    backend.rebuild_mesh(0)
    assert nodes_of(backend.export_two_level(), 0) != n_before             # (the mesh behind it moved)
    rebuilt = _visible(art, backend)
    assert 200 < (rebuilt[2][:, 1].view(np.int32) != 0).sum() < rebuilt[2].shape[0]      # (rays do hit something, and not all of them: word 1 = is_hit)
    for k, what in enumerate(("picture", "ArtStats::rays", "hit records")):
        assert np.array_equal(rebuilt[k], refitted[k]), what
    assert np.array_equal(rebuilt[0], flat_picture), "the flattened deformed scene's picture"


# ---- 3. other meshes' opened entry points -----------------------------------------------------------------------------------------------
def opened_scene(art):
    """four instances: mesh 1's two are large, mesh 0's two a tenth of their size; with inst_open 2 (eight entry points, the largest
    box opened first) the build opens mesh 1's instances and leaves mesh 0's whole"""
    A = R().placed(0, 4)
    m = R().mats(A).reshape(4, 3, 4).copy()
    for i, mesh in enumerate(R().mesh_of(A)):
        if mesh == 0:
            m[i, :, :3] *= F(0.1)
    return R().with_mats(R().mesh_of(A), m.reshape(4, 12))


def test_opened_entry_points_of_another_mesh_are_relocated(art, backend, options):
    A = opened_scene(art)
    B, qB = deformed(art, A, 0)
    hostA, hostB = host_build(art, "opened A", A, 2), host_build(art, "opened B", B, 2)
    owner = hostA["inst"][:, ref.INST].view(np.int32); root = hostA["inst"][:, ref.ROOT_ENTRY].view(np.int32)
    mesh = np.array(R().mesh_of(A))[owner]
    assert (root[mesh == 0] == 0).all() and (root[mesh == 1] != 0).any() and ((root[mesh == 1] & 15) == 0).any()      # mesh 0 whole; mesh 1 opened, at inner nodes too
    assert nodes_of(hostA, 0) != nodes_of(hostB, 0)
    options("inst_open", 2)
    backend.upload_scene(A)
    assert_same(backend.export_two_level(), dict(hostA, updated=0), "the upload is the host build")
    backend.refit_mesh_torch(0, gpu(qB))
    before = backend.export_two_level()
    want = _visible(art, backend)
    with pytest.raises(art.ArtError, match="inst_open"):
        backend.rebuild_mesh(1)
    assert_same(backend.export_two_level(), before, "a refused rebuild of the opened mesh")
    assert backend.mesh_rebuild_info().rebuilds == 0
    backend.rebuild_mesh(0)
    got = backend.export_two_level()
    delta = nodes_of(got, 0) - nodes_of(before, 0)
    assert delta != 0
    walk_all(got)
    inst = got["inst"].copy()
    behind = mesh == 1
    inst[behind, ref.NODE_BASE] = (inst[behind, ref.NODE_BASE].view(np.int32) - delta).view(np.uint32)
    inner = behind & ((inst[:, ref.QROOT] & np.uint32(0x80000000)) == 0)
    inst[inner, ref.QROOT] -= np.uint32((delta * 64) & 0xFFFFFFFF)
    assert np.array_equal(inst, before["inst"])                          # the entry points stay as built, but for the relocation
    after = _visible(art, backend)
    for k, what in enumerate(("picture", "ArtStats::rays", "hit records")):
        assert np.array_equal(after[k], want[k]), what
    # a move and a refit of the opened mesh against the new layout
    got, _ = R().moved(backend, got, R().mats(opened_scene(art)) * np.tile(np.array([1, 1, 1, 0.9], F), 3), "a move after the rebuild, opened")
    p1, _, i1 = R().verts(A, 1)
    R().refitted(backend, got, 1, i1, warp(p1), "a refit of the opened mesh after the rebuild")


# ---- 4. later updates ---------------------------------------------------------------------------------------------------------------------
def test_updates_after_the_rebuild_work_against_the_new_layout(art, backend, options):
    n = 12
    A = R().placed(0, n)
    B, qB = deformed(art, A, 0)
    p0, _, i0 = R().verts(A, 0)
    p1, _, i1 = R().verts(A, 1)
    q1 = warp(p1)
    End = R().variant(art, A, {1: (q1, None)})
    mA = R().mats(A)
    mC = mA * np.tile(np.array([1, 1, 1, 0.9], F), 3)                   # every instance a tenth closer to the origin: no pad has to grow
    options("inst_open", 1)
    backend.upload_scene(End)
    fresh = backend.export_two_level()
    backend.upload_scene(A)
    backend.refit_mesh_torch(0, gpu(qB))
    backend.rebuild_mesh(0)
    ex = backend.export_two_level()
    assert nodes_of(ex, 0) == nodes_of(host_build(art, ("B", n, 0), B), 0) != nodes_of(fresh, 0)
    ex, _ = R().moved(backend, ex, mC, "a move after the rebuild")
    ex, _ = R().refitted(backend, ex, 1, i1, q1, "a refit of the mesh behind the rebuilt one")
    ex, _ = R().refitted(backend, ex, 0, i0, p0, "a refit of the rebuilt mesh back to the uploaded vertices")
    ex, _ = R().moved(backend, ex, mA, "a move back")
    backend.rebuild_instances()
    backend.rebuild_mesh(0)
    backend.rebuild_mesh(1)
    got = backend.export_two_level()
    assert np.array_equal(bits(got["mesh_pad"]), bits(fresh["mesh_pad"]))   # (no move asked for a wider pad)
    assert_same(got, dict(fresh, updated=1), "the end state against a fresh upload")
    walk_all(got)
    assert backend.mesh_rebuild_info().rebuilds == 3 and backend.instance_rebuild_info().rebuilds == 1
    R().moved(backend, got, mC, "a move after the last rebuild")


# ---- 5. small shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["2_and_5_triangles", "single_mesh", "one_instance"])
def test_small_shapes(art, backend, options, shape):
    t = [R()._target(k) for k in range(3)]
    if shape == "2_and_5_triangles":
        meshes, insts, which = [R().grid_mesh(art, 2), R().grid_mesh(art, 5, amp=0.3)], [(0, t[0]), (1, t[1]), (0, t[2])], (0, 1)
    elif shape == "single_mesh":
        meshes, insts, which = [R().grid_mesh(art, 300)], [(0, t[0]), (0, t[1])], (0,)
    else:
        meshes, insts, which = [R().grid_mesh(art, 300), R().grid_mesh(art, 64, amp=0.3)], [(1, t[0])], (1,)
    options("inst_open", 1)

    def scene(ms):
        return R().custom(art, ms, insts)

    new = [dict(m, pos=warp(m["pos"], (2.0, 1.0, 0.5)) if k in which else m["pos"]) for k, m in enumerate(meshes)]
    backend.upload_scene(scene(new))
    fresh = backend.export_two_level()
    backend.upload_scene(scene(meshes))
    if shape == "one_instance":
        with pytest.raises(art.ArtError, match="no instance shows mesh 0"):
            backend.rebuild_mesh(0)
        with pytest.raises(art.ArtError, match="no instance shows mesh 0"):
            backend.mesh_tree_cost(0)
    for k in which:
        backend.refit_mesh_torch(k, gpu(new[k]["pos"]))
        backend.rebuild_mesh(k)
    if len(insts) > 1:
        backend.rebuild_instances()
    got = backend.export_two_level()
    if np.array_equal(bits(got["mesh_pad"]), bits(fresh["mesh_pad"])):
        assert_same(got, dict(fresh, updated=1), shape)
    else:                                                                 # (a pad that had to grow: everything the pad does not enter)
        for name in ("inst", "blas_tris", "tlas_tris", "mesh_base", "node_mesh", "mesh_box"):
            assert np.array_equal(got[name].view(np.uint32), fresh[name].view(np.uint32)), name
    walk_all(got)
    assert backend.mesh_rebuild_info().rebuilds == len(which)


# ---- 6. the cost figure --------------------------------------------------------------------------------------------------------------------
def _cost_numpy(nodes):
    from test_gpu_rebuild import _cost_ref
    return _cost_ref(np.asarray(nodes, F).reshape(-1), SimpleNamespace(node_width=4))


def _assert_cost(backend, m):
    """tests/test_gpu_rebuild.py's bound: the same positive binary64 terms on both sides, only the order of summation differs: 1e-9"""
    ex = backend.export_two_level()
    nb, nn = ref.mesh_slices(ex, m)[:2]
    want = _cost_numpy(ex["blas_nodes"][nb:nb + nn])
    tc = backend.mesh_tree_cost(m)
    got = (tc.root_area, tc.node_visits, tc.leaf_visits, tc.tri_tests)
    print("mesh %d tree cost: got %r, numpy %r" % (m, got, want[:4]))
    for g, w in zip(got, want[:4]):
        assert w > 0.0 and abs(g - w) <= 1e-9 * abs(w), (got, want)
    return got


def test_the_cost_figure_is_numpys_and_falls_across_the_rebuild(art, backend, options):
    A = R().placed(0, 12)
    B, qB = deformed(art, A, 0, STRONG)
    options("inst_open", 1)
    backend.upload_scene(B)
    fresh = [_assert_cost(backend, m) for m in (0, 1)]
    backend.upload_scene(A)
    for m in (0, 1):
        _assert_cost(backend, m)                                         # an uploaded tree, before any plan exists
    backend.refit_mesh_torch(0, gpu(qB))
    refitted = _assert_cost(backend, 0)
    other = _assert_cost(backend, 1)
    backend.rebuild_mesh(0)
    rebuilt = _assert_cost(backend, 0)
    print("node + leaf visits: refitted %.6f, rebuilt %.6f" % (refitted[1] + refitted[2], rebuilt[1] + rebuilt[2]))
    assert refitted[1] + refitted[2] > rebuilt[1] + rebuilt[2]
    assert rebuilt == fresh[0]                                           # the same tree: the same figure
    assert _assert_cost(backend, 1) == other == fresh[1]                 # (the mesh behind it, at its new place)


# ---- 7. refusals and counters --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(art, backend, options):
    from ada_ray_tracer_amd import scenes
    backend.upload_scene(scenes.synthetic_scene(500, 3))
    with pytest.raises(art.ArtError, match="art_rebuild_device"):
        backend.rebuild_mesh(0)
    with pytest.raises(art.ArtError, match="not instanced"):
        backend.mesh_tree_cost(0)
    options("inst_open", 1)
    t = [R()._target(k) for k in range(2)]
    backend.upload_scene(R().custom(art, [R().grid_mesh(art, 1), R().grid_mesh(art, 64)], [(0, t[0]), (1, t[1])]))
    with pytest.raises(art.ArtError, match="fewer than two triangles.*art_refit_mesh_device"):
        backend.rebuild_mesh(0)
    assert backend.export_two_level()["updated"] == 0                    # (refused before the plan was built)
    A = R().placed(0, 12)
    B, qB = deformed(art, A, 0)
    backend.upload_scene(A)
    for bad in (-1, 2):
        with pytest.raises(art.ArtError, match="out of range"):
            backend.rebuild_mesh(bad)
        with pytest.raises(art.ArtError, match="out of range"):
            backend.mesh_tree_cost(bad)
    pos = qB.copy(); pos[5, 2] = np.nan
    backend.refit_mesh_torch(0, gpu(pos), check=False)
    with pytest.raises(art.ArtError, match="vertex coordinate"):
        backend.synchronize()
    before = backend.export_two_level()
    cost = backend.mesh_tree_cost(0)                                     # (the figure has no bad-state refusal: emptied slots add nothing)
    with pytest.raises(art.ArtError, match=r"0 bad instance matrix\(es\) and 1 bad vertex"):
        backend.rebuild_mesh(0)
    with pytest.raises(art.ArtError, match=r"0 bad instance matrix\(es\) and 1 bad vertex"):
        backend.rebuild_mesh(1)
    assert_same(backend.export_two_level(), before, "refused with a bad vertex in force")
    assert backend.mesh_tree_cost(0).node_visits == cost.node_visits
    backend.refit_mesh_torch(0, gpu(qB))
    bad = R().mats(A).copy(); bad[3, 5] = np.nan
    backend.move_instances_torch(gpu(bad), check=False)
    with pytest.raises(art.ArtError, match="instance matrix"):
        backend.synchronize()
    before = backend.export_two_level()
    with pytest.raises(art.ArtError, match=r"1 bad instance matrix\(es\) and 0 bad vertex.*a good art_move_instances_device"):
        backend.rebuild_mesh(0)
    assert_same(backend.export_two_level(), before, "refused with a bad matrix in force")
    assert backend.mesh_rebuild_info().rebuilds == 0                     # a failed call is not counted
    backend.move_instances_torch(gpu(R().mats(A)))
    backend.rebuild_mesh(0)                                              # the good updates cleared it
    backend.synchronize()
    ri = backend.mesh_rebuild_info()
    assert ri.rebuilds == 1 and ri.host_ms >= ri.build_ms > 0.0
    backend.rebuild_instances()
    assert_same(backend.export_two_level(), dict(host_build(art, ("B", 12, 0), B), updated=1), "after the good updates")


# ---- 8. two contexts on one GPU, and the gcore refusal ---------------------------------------------------------------------------------------
SCRIPT = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import torch
import ctypes as C
import test_gpu_rebuild_mesh as T
out = {}
A = T.R().placed(0, 12)
B, qB = T.deformed(art, A, 0)
be = art.Backend(0)
L = be.lib
verts = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0); tri = (C.c_int * 3)(0, 1, 2)
L.gcore_init_and_clear()
L.gcore_instance_meshes(L.gcore_add_mesh_3f(verts, 3, tri, 3), (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1), 1)
L.gcore_commit_scene()
for name, call in (("gcore", lambda: be.rebuild_mesh(0)), ("gcore_cost", lambda: be.mesh_tree_cost(0))):
    try:
        call()
        out[name] = "accepted"
    except art.ArtError as e:
        out[name] = str(e)
L.gcore_destroy()
be.upload_scene(B)
ref = T._visible(art, be)
be.shutdown()
be = art.Backend(devices=[0, 0])
be.upload_scene(A)
T._visible(art, be)                                           # (the old shape rendered once on every context)
be.refit_mesh_torch(0, T.gpu(qB))
be.rebuild_mesh(0)
got = T._visible(art, be)
out["two_contexts"] = bool(all(np.array_equal(g, r) for g, r in zip(got, ref)))
out["rebuilds"] = be.mesh_rebuild_info().rebuilds
be.refit_mesh_torch(1, T.gpu(T.R().verts(A, 1)[0]))           # the second context's plan follows its own new layout
be.move_instances_torch(T.gpu(T.R().mats(A)))
got = T._visible(art, be)
out["two_contexts_updated_again"] = bool(all(np.array_equal(g, r) for g, r in zip(got, ref)))
be.shutdown()
print("RESULT " + json.dumps(out))
'''


def test_two_contexts_on_one_gpu_and_the_gcore_refusal(art):
    """art_init_devices([0, 0]) in a child process (the library is a process-wide singleton): every context builds its own tree; and
    the refusal that needs a fresh process, a scene committed through the gcore seam"""
    r = subprocess.run([sys.executable, "-c", SCRIPT, art.ROOT], capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(line[0][7:])
    assert "gcore_commit_scene" in out["gcore"] and "gcore_commit_scene" in out["gcore_cost"]
    assert out["two_contexts"] and out["rebuilds"] == 1 and out["two_contexts_updated_again"]
