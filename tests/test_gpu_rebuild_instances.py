"""art_rebuild_instance_tree_device on the GPU: after a move the instance tree is built again over the entry points as they lie in HBM.
With whole instances as entry points the result is the tree of a fresh upload at the new matrices and of the host build
(tests/hostsim.py), word for word; with opened instances every entry point is reached once and every box follows the rules of
tests/two_level_ref.py; nothing visible changes; later moves and mesh refits work against the new tree; the cost figure is numpy's.
Every comparison but the cost figure's (1e-9, tests/test_gpu_rebuild.py's bound) is exact."""
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
SEED = 0xADA5EED0 + 64
TRIS = 300
W, H = 64, 64
# (entry points, placement A, placement B) with whole instances as entry points.  Node counts of the instance tree by hostsim.two_level
# at placements 0 and 1: 2 -> 1 / 1, 4 -> 1 / 1 (one node holds four), 5 -> 2 / 2, 64 -> 30 / 29, 300 -> 142 / 130: the last two pairs move
# the meshes' quantised nodes
PAIRS = [(2, 0, 1), (4, 0, 1), (5, 0, 1), (64, 0, 1), (300, 0, 1)]
RELOCATING = (64, 300)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).cuda()


def mats(sd):
    return np.array([list(sd.desc.instances[i].m) for i in range(sd.desc.n_instances)], F)


def placed(k, n=12, tris=TRIS):
    from ada_ray_tracer_amd import scenes
    return scenes.instanced_scene(n, tris, seed=SEED + k)


def with_mats(sd, m, tris=TRIS):
    from ada_ray_tracer_amd import scenes
    return scenes.instanced_scene(0, tris, transforms=[(int(sd.desc.instances[i].mesh), np.asarray(m[i], F).reshape(3, 4)) for i in range(len(m))])


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


def assert_tree_equals(got, want, what):
    """the instance table, the instance tree, its proxies, its part of the merged array, the meshes' first nodes and the counts"""
    n_tlas = want["tlas_nodes"].shape[0]
    assert got["tlas_nodes"].shape[0] == n_tlas and got["qnodes"].shape == want["qnodes"].shape and got["n_inst"] == want["n_inst"], what
    for name in ("inst", "tlas_nodes", "tlas_tris", "mesh_base"):
        assert np.array_equal(bits(got[name]) if got[name].dtype == F else got[name], bits(want[name]) if want[name].dtype == F else want[name]), "%s: %s" % (what, name)
    assert np.array_equal(got["qnodes"][:n_tlas], want["qnodes"][:n_tlas]), "%s: qnodes of the instance tree" % what


def assert_meshes_untouched(after, before, what):
    """the meshes' arrays word for word, and their quantised nodes but for the relocation of the inner entry words"""
    for name in ("blas_nodes", "blas_tris", "mesh_pad", "mesh_box"):
        assert np.array_equal(bits(after[name]), bits(before[name])), "%s: %s" % (what, name)
    assert np.array_equal(after["node_mesh"], before["node_mesh"]), what
    na, nb = after["tlas_nodes"].shape[0], before["tlas_nodes"].shape[0]
    qa, qb = after["qnodes"][na:].copy(), before["qnodes"][nb:]
    e = qa.reshape(-1, 4, 4)[:, :, 2]
    inner = (e & np.uint32(0x80000000)) == 0
    e[inner] -= np.uint32(((na - nb) * 64) & 0xFFFFFFFF)
    assert np.array_equal(qa, qb), "%s: the meshes' quantised nodes" % what
    return na - nb


def walk(ex):
    """the exported two-level tree walked as the cooperative kernel does: the entry points in the order they are reached, every
    instance-tree node reached once and only from the instance tree"""
    n_tlas, n_entry = ex["tlas_nodes"].shape[0], ex["inst"].shape[0]
    seen = np.zeros(n_tlas, bool)
    found, todo = [], [0]
    while todo:
        n = todo.pop()
        assert 0 <= n < n_tlas and not seen[n], "node %d" % n
        seen[n] = True
        for j in range(4):
            e = int(ex["qnodes"][n, 4 * j + 2])
            ref_, cnt = int(ex["tlas_nodes"][n, 4 * j + 3:4 * j + 4].view(np.int32)[0]), int(ex["tlas_nodes"][n, 16 + 4 * j + 3:16 + 4 * j + 4].view(np.int32)[0])
            if e == 0x80000000:
                assert ref_ < 0
                continue
            if e & 0x80000000:
                assert (e & 15) == 15 and cnt == 1 and 0 <= ref_ < n_entry
                ent = (e & 0x7FFFFFF0) >> 4
                assert ent == int(ex["tlas_tris"][ref_, 9:10].view(np.int32)[0])         # (both walks name the same entry point)
                found.append(ent)
            else:
                assert e % 64 == 0 and cnt == 0 and e // 64 == ref_
                todo.append(e // 64)
    assert seen.all()
    return found


# ---- 1. tree identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ka,kb", PAIRS)
def test_the_rebuilt_tree_is_the_uploads_and_the_host_builds(art, backend, options, n, ka, kb):
    A, B = placed(ka, n), placed(kb, n)
    hostA, hostB = host_build(art, (n, ka), A), host_build(art, (n, kb), B)
    differ = hostA["tlas_nodes"].shape[0] != hostB["tlas_nodes"].shape[0]
    assert differ == (n in RELOCATING)                                  # (picked on the CPU: these pairs exercise the relocation)
    options("inst_open", 1)
    backend.upload_scene(B)
    fresh = backend.export_two_level()
    backend.upload_scene(A)
    backend.move_instances_torch(gpu(mats(B)))
    before = backend.export_two_level()
    assert before["tlas_nodes"].shape[0] == hostA["tlas_nodes"].shape[0]
    backend.rebuild_instances()
    got = backend.export_two_level()
    assert got["inst"].shape[0] == n and got["updated"] == 1
    assert_tree_equals(got, fresh, "against a fresh upload")
    assert_tree_equals(got, hostB, "against the host build")
    shift = assert_meshes_untouched(got, before, "against the export before the rebuild")
    assert (shift != 0) == differ
    assert sorted(walk(got)) == list(range(n))
    ri = backend.instance_rebuild_info()
    assert ri.rebuilds == 1 and ri.gather_ms > 0.0 and ri.build_ms > 0.0 and ri.host_ms >= ri.build_ms


def host_tree_of_proxies(art, ex, kw):
    """the host builder's instance tree over the proxies of the export ex: (packets, proxy records with word 9 = the entry point)"""
    owner = ex["inst"][:, ref.INST].view(np.int32); root = ex["inst"][:, ref.ROOT_ENTRY].view(np.int32)
    order = np.lexsort((root, owner))                                    # the upload's proxy order: by (instance, root_entry)
    ids = ex["tlas_tris"][:, 9].view(np.int32)
    rec_of = np.empty(ids.size, np.int64); rec_of[ids] = np.arange(ids.size)
    pos = ex["tlas_tris"][rec_of[order], :9].reshape(-1, 3).copy()
    idx = np.arange(pos.shape[0], dtype=np.int32).reshape(-1, 3)
    flat = art.SceneDesc(meshes=[dict(mode=art.MESH_CLOSEST, pos=pos, nrm=np.tile(np.array([0, 1, 0], F), (pos.shape[0], 1)), idx=idx,
                                      matid=np.ones(idx.shape[0], np.int32))], **kw)
    hostsim.set_bvh_param(art, "max_leaf", 1)
    try:
        nodes, tris, info = hostsim.bvh(art, flat)
    finally:
        hostsim.set_bvh_param(art, "max_leaf", 8)
    assert info["width"] == 4
    tris = tris.reshape(-1, 12).copy()
    tris[:, 9] = order[tris[:, 9].view(np.int32)].astype(np.int32).view(F)
    return nodes.reshape(-1, 32), tris


def assert_is_host_tree(art, got, proxies_of, kw, what):
    nodes, tris = host_tree_of_proxies(art, proxies_of, kw)
    assert np.array_equal(bits(got["tlas_nodes"]), bits(nodes)), what + ": packets"
    assert np.array_equal(bits(got["tlas_tris"]), bits(tris)), what + ": proxy records"


# ---- 2. opened entry points --------------------------------------------------------------------------------------------------------------
def test_opened_entry_points_are_all_reached_once_and_the_boxes_follow_the_rules(art, backend, options):
    """inst_open = 8 on an interpenetrating cluster.  hostsim.bvh with max_leaf = 1 DOES reproduce the instance tree of an unmoved upload
    from its proxies (fed as the triangles of a flat mesh in the upload's proxy order: packets, records and ids agree word for word,
    checked below on the upload itself), so the rebuilt tree is held to that host build of the moved proxies too."""
    from ada_ray_tracer_amd import scenes
    n = 12
    A = scenes.instanced_cluster(n, TRIS)
    mB = mats(A).reshape(n, 3, 4).copy()
    mB[:, :, 3] = np.roll(mB[:, :, 3], 5, axis=0)                        # the instances swap places: still interpenetrating
    options("inst_open", 8)
    backend.upload_scene(A)
    up = backend.export_two_level()
    n_entry = up["inst"].shape[0]
    assert n_entry > 4 * n
    assert_is_host_tree(art, up, up, A._kw, "the upload's own tree from its proxies")
    backend.rebuild_instances()                                          # unmoved: the builder reproduces the upload's tree from its proxies
    same = backend.export_two_level()
    for name in ref.ARRAYS:
        assert np.array_equal(same[name].view(np.uint32), up[name].view(np.uint32)), name
    backend.move_instances_torch(gpu(mB.reshape(n, 12)))
    before = backend.export_two_level()
    backend.rebuild_instances()
    got = backend.export_two_level()
    assert sorted(walk(got)) == list(range(n_entry))
    assert_is_host_tree(art, got, before, A._kw, "the rebuilt tree from the moved proxies")
    shift = assert_meshes_untouched(got, before, "opened")
    inst = got["inst"].copy()
    inner = (inst[:, ref.QROOT] & np.uint32(0x80000000)) == 0
    inst[inner, ref.QROOT] -= np.uint32((shift * 64) & 0xFFFFFFFF)
    assert np.array_equal(inst, before["inst"])                          # the entry points stay as built
    assert np.array_equal(np.sort(got["tlas_tris"].view(np.uint32), axis=0), np.sort(before["tlas_tris"].view(np.uint32), axis=0))      # the same proxies
    ref.assert_equal(got, ref.move(got, mB.reshape(n, 12)), "a node refit of the rebuilt tree changes no word")


# ---- 3. nothing visible changes ---------------------------------------------------------------------------------------------------------
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
    occ = backend.occluded_torch(o, d).cpu().numpy()
    assert st.lost_paths == 0
    return bits(accum).copy(), int(st.rays), hits, occ


@pytest.mark.parametrize("kernel", ["coop", "coop_stack_cap_3", "one_ray_per_lane"])
def test_picture_hits_and_ray_count_do_not_change(art, backend, options, kernel):
    n = 64
    A, B = placed(0, n), placed(1, n)
    options("inst_coop", 0 if kernel == "one_ray_per_lane" else 1)
    options("lds_stack_cap", 3 if kernel == "coop_stack_cap_3" else 0)
    backend.upload_scene(B)
    want = _visible(art, backend)
    backend.upload_scene(A)
    backend.move_instances_torch(gpu(mats(B)))
    moved = _visible(art, backend)
    n_before = backend.export_two_level()["tlas_nodes"].shape[0]
    backend.rebuild_instances()
    assert backend.export_two_level()["tlas_nodes"].shape[0] != n_before   # (the meshes' nodes moved)
    rebuilt = _visible(art, backend)
    assert 200 < want[3].sum() < want[3].size                            # (rays do hit something, and not all of them)
    for k, what in enumerate(("picture", "ArtStats::rays", "hit records", "occlusion")):
        assert np.array_equal(moved[k], want[k]), "moved: " + what
        assert np.array_equal(rebuilt[k], want[k]), "rebuilt: " + what


# ---- 4. updates after a rebuild ---------------------------------------------------------------------------------------------------------
def test_a_move_and_a_mesh_refit_after_the_rebuild_equal_the_reference(art, backend, options):
    import test_gpu_two_level_reference as R
    n = 64
    A, B, Cc = placed(0, n), placed(1, n), placed(2, n)
    options("inst_open", 1)
    backend.upload_scene(A)
    backend.move_instances_torch(gpu(mats(B)))
    backend.rebuild_instances()
    ex = backend.export_two_level()
    assert ex["tlas_nodes"].shape[0] != host_build(art, (n, 0), A)["tlas_nodes"].shape[0]
    ex, _ = R.moved(backend, ex, mats(Cc), "a move after the rebuild")
    pos, nrm, idx, uv, matid = A._mesh_arrays[1]
    p2 = (np.asarray(pos, F) * F(1.3) + F(0.05)).astype(F)
    R.refitted(backend, ex, 1, idx, p2, "a mesh refit after the rebuild")


def test_move_rebuild_move_rebuild_equals_a_fresh_upload(art, backend, options):
    n = 64
    A, B, Cc = placed(0, n), placed(1, n), placed(2, n)
    options("inst_open", 1)
    backend.upload_scene(Cc)
    fresh = backend.export_two_level()
    backend.upload_scene(A)
    backend.move_instances_torch(gpu(mats(B)))
    backend.rebuild_instances()
    backend.move_instances_torch(gpu(mats(Cc)))
    backend.rebuild_instances()
    got = backend.export_two_level()
    assert_tree_equals(got, fresh, "move, rebuild, move, rebuild")
    assert_tree_equals(got, host_build(art, (n, 2), Cc), "move, rebuild, move, rebuild, against the host build")
    # the meshes' pads may have grown on the way (they only grow): their boxes are never narrower than the upload's
    assert (got["mesh_pad"] >= fresh["mesh_pad"]).all() and np.array_equal(bits(got["blas_tris"]), bits(fresh["blas_tris"]))
    same = got["mesh_pad"] == fresh["mesh_pad"]
    if same.all():
        ref.assert_equal(got, dict(fresh, updated=1), "every array")
    assert backend.instance_rebuild_info().rebuilds == 2


# ---- 5. cost ----------------------------------------------------------------------------------------------------------------------------
def _cost_numpy(tlas_nodes):
    from test_gpu_rebuild import _cost_ref
    return _cost_ref(np.asarray(tlas_nodes, F).reshape(-1), SimpleNamespace(node_width=4))


def _assert_cost(backend):
    """tests/test_gpu_rebuild.py's bound: the same positive binary64 terms on both sides, only the order of summation differs: 1e-9"""
    want = _cost_numpy(backend.export_two_level()["tlas_nodes"])
    tc = backend.instance_tree_cost()
    got = (tc.root_area, tc.node_visits, tc.leaf_visits, tc.tri_tests)
    print("instance tree cost: got %r, numpy %r" % (got, want[:4]))
    for g, w in zip(got, want[:4]):
        assert w > 0.0 and abs(g - w) <= 1e-9 * abs(w), (got, want)
    assert got[2] == got[3]                                              # (one entry point per leaf)
    return got


def scattering(n=64):
    """(A, B): B is placement 0, A the same instances pulled into a cluster around the middle of the box and shuffled"""
    B = placed(0, n)
    mB = mats(B).reshape(n, 3, 4)
    c = np.array([0.0, 2.3, 2.3], F)
    mA = mB.copy()
    mA[:, :, 3] = c + F(0.25) * (mB[np.random.default_rng(5).permutation(n), :, 3] - c)
    return with_mats(B, mA.reshape(n, 12)), B


def test_the_cost_figure_is_numpys_and_falls_across_the_rebuild_of_a_scattered_cluster(art, backend, options):
    A, B = scattering()
    options("inst_open", 1)
    exA = host_build(art, "scatter A", A)
    refitted_cpu = _cost_numpy(ref.move(exA, mats(B))["tlas_nodes"])
    rebuilt_cpu = _cost_numpy(host_build(art, (64, 0), B)["tlas_nodes"])
    print("CPU figures: refitted %r, rebuilt %r" % (refitted_cpu[:4], rebuilt_cpu[:4]))
    assert refitted_cpu[1] + refitted_cpu[2] > rebuilt_cpu[1] + rebuilt_cpu[2]      # (the pair was chosen for it)
    backend.upload_scene(A)
    _assert_cost(backend)                                                # an uploaded tree
    backend.move_instances_torch(gpu(mats(B)))
    moved = _assert_cost(backend)                                        # a refitted tree
    backend.rebuild_instances()
    rebuilt = _assert_cost(backend)                                      # a rebuilt tree
    for g, w in zip(moved, refitted_cpu[:4]):
        assert abs(g - w) <= 1e-9 * abs(w)
    for g, w in zip(rebuilt, rebuilt_cpu[:4]):
        assert abs(g - w) <= 1e-9 * abs(w)
    assert moved[1] + moved[2] > rebuilt[1] + rebuilt[2]


# ---- 6. refusals and atomicity ----------------------------------------------------------------------------------------------------------
def test_refusals_and_a_failed_call_leaves_everything_as_it_was(art, backend, options):
    from ada_ray_tracer_amd import scenes
    n = 12
    A, B = placed(0, n), placed(1, n)
    backend.upload_scene(scenes.synthetic_scene(500, 3))
    with pytest.raises(art.ArtError, match="not instanced"):
        backend.rebuild_instances()
    with pytest.raises(art.ArtError, match="not instanced"):
        backend.instance_tree_cost()
    options("inst_open", 1)
    backend.upload_scene(placed(0, 1))
    with pytest.raises(art.ArtError, match="fewer than two entry points"):
        backend.rebuild_instances()
    assert backend.export_two_level()["updated"] == 0                    # (refused before the plan was built)
    backend.upload_scene(A)
    bad = mats(B).copy(); bad[3, 5] = np.nan; bad[7, 0] = np.inf
    backend.move_instances_torch(gpu(bad), check=False)
    with pytest.raises(art.ArtError, match="2 instance matrix"):
        backend.synchronize()
    before = backend.export_two_level()
    cost = backend.instance_tree_cost()
    with pytest.raises(art.ArtError, match=r"2 bad instance matrix\(es\) and 0 bad vertex.*a good art_move_instances_device"):
        backend.rebuild_instances()
    after = backend.export_two_level()
    for name in ref.ARRAYS:
        assert np.array_equal(after[name].view(np.uint32), before[name].view(np.uint32)), name
    assert backend.instance_tree_cost().node_visits == cost.node_visits
    assert backend.instance_rebuild_info().rebuilds == 0                 # a failed call is not counted
    pos = np.asarray(A._mesh_arrays[0][0], F).copy(); pos[5, 2] = np.nan
    backend.move_instances_torch(gpu(mats(B)))
    backend.refit_mesh_torch(0, gpu(pos), check=False)
    with pytest.raises(art.ArtError, match="vertex coordinate"):
        backend.synchronize()
    with pytest.raises(art.ArtError, match=r"0 bad instance matrix\(es\) and 1 bad vertex"):
        backend.rebuild_instances()
    backend.refit_mesh_torch(0, gpu(np.asarray(A._mesh_arrays[0][0], F)))
    backend.rebuild_instances()                                          # a good refit cleared it
    backend.synchronize()
    got = backend.export_two_level()
    assert_tree_equals(got, host_build(art, (n, 1), B), "after the good updates")
    assert backend.instance_rebuild_info().rebuilds == 1


# ---- 7. two contexts on one GPU, and the gcore refusal ---------------------------------------------------------------------------------------
SCRIPT = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import torch
import ctypes as C
import test_gpu_rebuild_instances as T
out = {}
A, B = T.placed(0, 64), T.placed(1, 64)
be = art.Backend(0)
L = be.lib
verts = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0); tri = (C.c_int * 3)(0, 1, 2)
L.gcore_init_and_clear()
L.gcore_instance_meshes(L.gcore_add_mesh_3f(verts, 3, tri, 3), (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1), 1)
L.gcore_commit_scene()
for name, call in (("gcore", be.rebuild_instances), ("gcore_cost", be.instance_tree_cost)):
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
T._visible(art, be)                                           # (the old placement rendered once on every context)
be.move_instances_torch(T.gpu(T.mats(B)))
be.rebuild_instances()
got = T._visible(art, be)
out["two_contexts"] = bool(all(np.array_equal(g, r) for g, r in zip(got, ref)))
out["rebuilds"] = be.instance_rebuild_info().rebuilds
be.move_instances_torch(T.gpu(T.mats(A)))                     # the second context's plan follows its own new tree
be.move_instances_torch(T.gpu(T.mats(B)))
got = T._visible(art, be)
out["two_contexts_moved_again"] = bool(all(np.array_equal(g, r) for g, r in zip(got, ref)))
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
    assert out["two_contexts"] and out["rebuilds"] == 1 and out["two_contexts_moved_again"]
