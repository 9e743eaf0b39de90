"""art_move_instances_device and art_refit_mesh_device against an independent reference (tests/two_level_ref.py, plain numpy, itself
checked against the host builder in tests/test_two_level_reference_host.py): every array of the two-level scene in HBM
(Backend.export_two_level(): the instance table, the instance tree's packets and proxies, the meshes' packets and records, the merged
quantised nodes, the meshes' pads and boxes) word for word after moves and mesh refits, at the shapes at which the update kernels take
another path -- more than one wave and block of k_move_matrices, an instance tree of three levels, both variants of k_move_entry_boxes
and the boundary between them, pads that rise for one mesh only, bad matrices and bad vertices -- and the hits of rays aimed at the
instances against the brute-force oracle of the flattened target.  Every comparison is exact."""
import json
import subprocess
import sys

import numpy as np
import pytest

import conv
import hostsim
import orc
import refit_ref
import two_level_ref as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 0xADA5EED0 + 64
TRIS = 40


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).cuda()


def mats(sd):
    return np.array([list(sd.desc.instances[i].m) for i in range(sd.desc.n_instances)], F)


def mesh_of(sd):
    return [int(sd.desc.instances[i].mesh) for i in range(sd.desc.n_instances)]


def placed(k, n=12, tris=TRIS):
    from ada_ray_tracer_amd import scenes
    return scenes.instanced_scene(n, tris, seed=SEED + k)


def with_mats(meshes, m, tris=TRIS):
    """the two prototype meshes, instance i showing meshes[i] under m[i]"""
    from ada_ray_tracer_amd import scenes
    return scenes.instanced_scene(0, tris, transforms=[(meshes[i], np.asarray(m[i], F).reshape(3, 4)) for i in range(len(m))])


def swapped(k, n):
    """placement k's matrices, the translations permuted among the instances (test_instances_that_swap_places)"""
    m = mats(placed(k, n)).reshape(n, 3, 4).copy()
    m[:, :, 3] = np.roll(m[:, :, 3], 5, axis=0)
    return m.reshape(n, 12)


def grid_mesh(art, n, amp=0.15):
    """the first n triangles of a bumpy grid over [-1, 1]^2"""
    m = max(1, int(np.ceil((n / 2.0) ** 0.5)))
    g = np.linspace(-1.0, 1.0, m + 1)
    X, Z = np.meshgrid(g, g, indexing="ij")
    pos = np.stack([X, amp * np.sin(3.0 * X) * np.cos(2.0 * Z), Z], -1).reshape(-1, 3).astype(F)
    nrm = np.tile(np.array([0.0, 1.0, 0.0], F), (pos.shape[0], 1))
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    a_ = (i * (m + 1) + j).ravel(); b_ = ((i + 1) * (m + 1) + j).ravel(); c_ = (i * (m + 1) + j + 1).ravel(); d_ = ((i + 1) * (m + 1) + j + 1).ravel()
    idx = np.stack([np.stack([a_, c_, b_], 1), np.stack([b_, c_, d_], 1)], 1).reshape(-1, 3).astype(np.int32)[:n]
    assert idx.shape[0] == n
    return dict(mode=art.MESH_CLOSEST, pos=pos, nrm=nrm, idx=np.ascontiguousarray(idx), matid=(1 + (np.arange(n) % 3)).astype(np.int32))


def custom(art, meshes, insts):
    """the Cornell box and lights of scenes.instanced_scene around meshes of the test's own"""
    return art.SceneDesc(meshes=meshes, instances=[(mi, np.asarray(m, F).ravel()) for mi, m in insts], **placed(0, 1)._kw)


def variant(art, sd, meshes):
    """sd with the (pos, nrm) of the meshes in `meshes` replaced"""
    ms = []
    for k, (pos, nrm, idx, uv, matid) in enumerate(sd._mesh_arrays):
        p, n = meshes.get(k, (pos, nrm))
        ms.append(dict(mode=art.MESH_CLOSEST, pos=p, nrm=nrm if n is None else n, idx=idx, uv=uv, matid=matid))
    inst = [(int(sd.desc.instances[i].mesh), list(sd.desc.instances[i].m)) for i in range(sd.desc.n_instances)]
    return art.SceneDesc(meshes=ms, instances=inst, **sd._kw)


@pytest.fixture
def options(backend):
    yield backend.set_option
    backend.set_option("inst_open", 0)


def upload(backend, sd):
    backend.upload_scene(sd)
    ex = backend.export_two_level()
    assert ex["updated"] == 0 and ex["n_inst"] == sd.desc.n_instances
    return ex


def moved(backend, ex, m, what, bad=0):
    """move to m on top of the export ex; the new export equals the reference's; returns (export, the reference's details)"""
    backend.move_instances_torch(gpu(m), check=False)
    got = backend.export_two_level()
    want, d = ref.move(ex, m, details=True)
    assert got["updated"] == 1 and int((~d["ok"]).sum()) == bad
    ref.assert_equal(got, want, what)
    return got, d


def refitted(backend, ex, mesh, idx, pos, what, nrm=None):
    backend.refit_mesh_torch(mesh, gpu(pos), None if nrm is None else gpu(nrm), check=False)
    got = backend.export_two_level()
    want, d = ref.refit_mesh(ex, mesh, idx, pos, details=True)
    ref.assert_equal(got, want, what)
    return got, d


# ---- a. a move to where the instances are ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst_open", [0, 8])
def test_a_move_to_where_the_instances_are_changes_no_word(art, backend, options, inst_open):
    options("inst_open", inst_open)
    sd = placed(0)
    ex = upload(backend, sd)
    if inst_open == 8:
        assert ex["inst"].shape[0] > 12
    backend.move_instances_torch(gpu(mats(sd)))
    got = backend.export_two_level()
    assert got["updated"] == 1
    ref.assert_equal(got, ex, "unmoved")
    assert backend.move_info().repads == 0


# ---- b. moved scenes, word for word ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 300])
def test_moved_instances_equal_the_reference(art, backend, options, n):
    """1 .. 300 instances: below, at and above the wave (64) and the block (128) of k_move_matrices / k_move_pads_inst; at 300 the
    instance tree has three levels, so an inner child takes its box from a node that an earlier launch refitted, twice over"""
    options("inst_open", 1)
    ex = upload(backend, placed(0, n))
    if n == 300:
        assert ref.tlas_levels(ex) >= 3
    m1 = swapped(1, n)
    got, _ = moved(backend, ex, m1, "%d instances, first move" % n)
    assert not np.array_equal(got["tlas_nodes"], ex["tlas_nodes"])
    moved(backend, got, swapped(2, n), "%d instances, second move" % n)
    mi = backend.move_info()
    assert mi.moves == 2 and mi.bad_matrices == 0


@pytest.mark.parametrize("inst_open", [1, 8, 1000])
def test_opened_instances_equal_the_reference(art, backend, options, inst_open):
    """65 instances opened into 8 and into as many entry points as there are (1000): entry points outnumber instances, and an entry
    point gathers several record ranges"""
    options("inst_open", inst_open)
    ex = upload(backend, placed(0, 65))
    n_entry = ex["inst"].shape[0]
    assert n_entry == 65 if inst_open == 1 else n_entry > 4 * 65
    got, _ = moved(backend, ex, swapped(1, 65), "inst_open %d, first move" % inst_open)
    moved(backend, got, swapped(2, 65), "inst_open %d, second move" % inst_open)


def _target(k):
    return mats(placed(k, 1))[0]


@pytest.mark.parametrize("records", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_one_instance_of_a_grid_equals_the_reference(art, backend, options, records):
    """one entry point over `records` records: k_move_entry_boxes<64> up to 64 (one wave, its last lanes idle or a second trip of the
    strided loop), <256> from 65 on (the cross-wave reduction; 255 / 256 / 257: the tail of its strided loop)"""
    options("inst_open", 1)
    ex = upload(backend, custom(art, [grid_mesh(art, records)], [(0, _target(0))]))
    assert ex["blas_tris"].shape[0] == records and ex["inst"].shape[0] == 1
    got, _ = moved(backend, ex, _target(1)[None], "%d records, first move" % records)
    moved(backend, got, _target(2)[None], "%d records, second move" % records)


@pytest.mark.parametrize("records", [(63, 65), (64, 65)])
def test_two_instances_on_each_side_of_the_variant_boundary(art, backend, options, records):
    """two entry points over 128 records (= 64 per entry point: the one-wave variant) and over 129 (the 256-lane variant)"""
    options("inst_open", 1)
    ex = upload(backend, custom(art, [grid_mesh(art, records[0]), grid_mesh(art, records[1], amp=0.3)], [(0, _target(0)), (1, _target(3))]))
    assert ex["blas_tris"].shape[0] == sum(records) and ex["inst"].shape[0] == 2
    got, _ = moved(backend, ex, np.stack([_target(1), _target(4)]), "%s records, first move" % (records,))
    moved(backend, got, np.stack([_target(2), _target(5)]), "%s records, second move" % (records,))


def awkward(how):
    tr = hostsim.awkward_instances()
    meshes = [mi for mi, _ in tr]
    m = np.array([M.ravel() for _, M in tr], np.float64)
    if how == "far":
        m[0, 3] += 1.0e5; m[2, 11] -= 1.0e5                                      # two instances a translation of 1e5 away
    elif how == "huge":
        m[6].reshape(3, 4)[:, :3] *= 1.0e3                                       # the large instance a thousand times larger
    return meshes, m.astype(F)


@pytest.mark.parametrize("how", ["awkward", "far", "huge"])
@pytest.mark.parametrize("inst_open", [1, 8])
def test_a_move_to_awkward_instances_equals_the_reference(art, backend, options, how, inst_open):
    """the identity, a mirror image, coincident, sheared, tiny (1e-3: its mesh's pad rises a thousandfold) and large instances; far: a
    translation of 1e5 (world boxes whose pad is all rounding); huge: a scale of 1e3 (the extent E and with it every pad rises)"""
    options("inst_open", inst_open)
    meshes, m = awkward(how)
    ex = upload(backend, with_mats(meshes, mats(placed(0, len(meshes)))))
    got, d = moved(backend, ex, m, how)
    assert 0 in d["repadded"] and got["mesh_pad"][0] > ex["mesh_pad"][0]
    if how == "huge":
        assert d["E"] > float(ex["scene_extent"]) and d["repadded"] == [0, 1]
    moved(backend, got, mats(placed(1, len(meshes))), how + ", back to ordinary matrices")


def test_a_move_that_raises_one_meshs_pad_only(art, backend, options):
    options("inst_open", 1)
    A = placed(0)
    ex = upload(backend, A)
    m = mats(A)
    m[0].reshape(3, 4)[:, :3] *= F(1.0e-3)                                       # instance 0 shows mesh 0
    got, d = moved(backend, ex, m, "one pad")
    assert got["mesh_pad"][0] > ex["mesh_pad"][0] and got["mesh_pad"][1].view(np.uint32) == ex["mesh_pad"][1].view(np.uint32)
    nb, nn, _, _, qb = ref.mesh_slices(ex, 1)
    assert np.array_equal(got["blas_nodes"][nb:nb + nn].view(np.uint32), ex["blas_nodes"][nb:nb + nn].view(np.uint32))
    assert np.array_equal(got["qnodes"][qb:qb + nn], ex["qnodes"][qb:qb + nn])
    nb, nn, _, _, qb = ref.mesh_slices(ex, 0)
    assert not np.array_equal(got["blas_nodes"][nb:nb + nn].view(np.uint32), ex["blas_nodes"][nb:nb + nn].view(np.uint32))
    assert backend.move_info().repads == 1 and d["repadded"] == [0]


def leaf_company(ex):
    """per instance: the instance tree node whose slot names its proxy, and how many leaf slots that node has"""
    nodes = ex["tlas_nodes"]
    r = nodes[:, 3:16:4].view(np.int32); c = nodes[:, 19:32:4].view(np.int32)
    ids = ex["tlas_tris"][:, 9].view(np.int32)
    node_of = np.zeros(ids.size, np.int64)
    for nd in range(nodes.shape[0]):
        for j in range(4):
            if r[nd, j] >= 0 and c[nd, j] > 0:
                node_of[ids[r[nd, j]:r[nd, j] + c[nd, j]]] = nd
    leaves = ((r >= 0) & (c > 0)).sum(axis=1)
    return node_of, leaves[node_of]


@pytest.mark.parametrize("count", [1, 3])
def test_bad_matrices_empty_what_the_reference_empties(art, backend, options, count):
    """NaN, all zeros and a reach beyond 1e18, on one and on three of 65 instances.  The instance tree's leaves hold one proxy each, so
    the company that matters is the node: the victims are the instance whose node has the fewest leaf slots (one bad child empties
    most of it) and, for three, also two that share a node with good ones."""
    options("inst_open", 1)
    A = placed(0, 65)
    ex = upload(backend, A)
    node_of, company = leaf_company(ex)
    lone = int(np.argmin(company))
    shared = [int(i) for i in np.argsort(-company, kind="stable") if i != lone][:2]
    assert company[shared[0]] >= 2 and node_of[shared[0]] != node_of[lone]
    print("leaf slots in the victims' nodes:", company[lone], company[shared])
    m = swapped(1, 65)
    bad = m.copy()
    if count == 1:
        bad[lone, 6] = np.nan
        victims = [lone]
    else:
        bad[lone] = 0.0; bad[shared[0], 1] = np.inf; bad[shared[1], 7] = F(2.0e18)
        victims = [lone] + shared
    got, d = moved(backend, ex, bad, "%d bad" % count, bad=count)
    assert sorted(np.nonzero(~d["ok"])[0].tolist()) == sorted(victims)
    with pytest.raises(art.ArtError, match="%d instance matrix" % count):
        backend.synchronize()
    backend.synchronize()
    assert np.isinf(got["tlas_nodes"][:, :16].reshape(-1, 4, 4)[:, :, :3]).any()      # (empty boxes did appear)
    got2, _ = moved(backend, got, bad, "%d bad, again" % count, bad=count)      # the proxies keep the words of the last good box
    with pytest.raises(art.ArtError, match="%d instance matrix" % count):
        backend.synchronize()
    back, _ = moved(backend, got2, m, "a good move after the bad one")
    backend.synchronize()
    assert np.isfinite(back["tlas_nodes"][:, :16].reshape(-1, 4, 4)[:, :, :3][back["tlas_nodes"][:, 3:16:4].view(np.int32) >= 0]).all()
    assert backend.move_info().bad_matrices == 2 * count


# ---- c. mesh refits -------------------------------------------------------------------------------------------------------------------
def verts(sd, mesh):
    return sd._mesh_arrays[mesh][0].copy(), sd._mesh_arrays[mesh][1].copy(), sd._mesh_arrays[mesh][2]


@pytest.mark.parametrize("inst_open", [1, 8])
def test_mesh_refits_equal_the_reference(art, backend, options, inst_open):
    options("inst_open", inst_open)
    A = placed(0)
    ex = upload(backend, A)
    p0, n0, i0 = verts(A, 0)
    p1, n1, i1 = verts(A, 1)
    got, d = refitted(backend, ex, 1, i1, (p1 * F(0.5)).astype(F), "the grid shrinks")
    assert not d["repadded"] and not np.array_equal(got["mesh_box"][1], ex["mesh_box"][1])
    inside = (p0 * np.array([1.0, 0.7, 1.0], F)).astype(F)
    got, d = refitted(backend, got, 0, i0, inside, "the torus stays inside its box")
    assert not d["repadded"]
    grown = (p0 * F(40.0)).astype(F)                                             # 40 x 1 x 0.6: past the camera at 12.5, the scene's extent
    before = got
    got, d = refitted(backend, got, 0, i0, grown, "the torus grows past the scene's extent")
    assert d["E"] > float(ex["scene_extent"]) and 1 in d["repadded"]
    assert got["mesh_pad"][1] > before["mesh_pad"][1]                            # (the OTHER mesh's pad; its value is the reference's: refitted())
    got, _ = refitted(backend, got, 0, i0, p0, "and back")
    nb, nn, tb, nrec, _ = ref.mesh_slices(ex, 0)
    refit_ref.diff_report(got["blas_tris"][tb:tb + nrec], ex["blas_tris"][tb:tb + nrec], "the torus' records back home")
    same, _ = refitted(backend, got, 0, i0, p0, "new normals only", nrm=(-n0).astype(F))
    ref.assert_equal(same, got, "new normals only: the tree")
    ri = backend.mesh_refit_info()
    assert ri.refits == 5 and ri.bad_vertices == 0 and ri.repads >= 1 and backend.move_info().repads == 0


def test_refits_and_moves_in_sequence(art, backend, options):
    options("inst_open", 8)
    A = placed(0)
    p0, _, i0 = verts(A, 0)
    p1, _, i1 = verts(A, 1)
    d0 = (p0 * np.array([1.6, 0.8, 1.2], F)).astype(F); d1 = (p1 * np.array([0.9, 2.5, 0.9], F)).astype(F)
    ex = upload(backend, A)                                                      # refit -> move -> refit
    got, _ = refitted(backend, ex, 0, i0, d0, "refit")
    got, _ = moved(backend, got, swapped(1, 12), "refit, move")
    got, _ = refitted(backend, got, 1, i1, d1, "refit, move, refit")
    ex = upload(backend, A)                                                      # move -> refit: the move builds the plan
    got, _ = moved(backend, ex, swapped(2, 12), "move")
    refitted(backend, got, 0, i0, d0, "move, refit")


def test_bad_vertices_empty_what_the_reference_empties(art, backend, options):
    """NaN, inf and 3e18, two coordinates of one vertex, and a vertex no triangle uses (tests/test_gpu_refit_reference.py item 4): the
    records take the bad corners, the slots above them and the entry points above those are empty where the reference empties them"""
    options("inst_open", 8)
    A = placed(0)
    p0, n0, i0 = verts(A, 0)
    extra = p0.shape[0]
    p0x = np.concatenate([p0, np.array([[0.1, 0.2, 0.3]], F)]); n0x = np.concatenate([n0, np.array([[0.0, 1.0, 0.0]], F)])
    sd = variant(art, A, {0: (p0x, n0x)})
    assert not (i0 == extra).any()
    ex = upload(backend, sd)
    nt = i0.shape[0]
    bad = (p0x * np.array([1.2, 0.9, 1.1], F)).astype(F)
    good = bad.copy()
    bad[i0[3, 0], 1] = np.nan; bad[i0[3, 0], 2] = np.nan                         # two coordinates of one vertex
    bad[i0[nt // 2, 1], 0] = np.inf
    bad[i0[nt - 1, 2], 2] = F(-3.0e18)
    bad[extra, 1] = np.inf
    n_bad = int((~(np.abs(bad) <= 1e18).all(axis=1)).sum())
    assert n_bad == 4
    got, d = refitted(backend, ex, 0, i0, bad, "bad vertices")
    with pytest.raises(art.ArtError, match="art_refit_mesh_device: 4 vertex coordinate"):
        backend.synchronize()
    backend.synchronize()
    owner = got["inst"][:, ref.INST].view(np.int32)
    on_torus = np.array(d["inst_mesh"])[owner] == 0
    empty = ~(d["entry_lo"][:, 0] <= d["entry_hi"][:, 0])
    assert empty.any() and not empty[~on_torus].any() and not empty[on_torus].all()      # some of the torus' entry points, none of the grid's
    assert np.isinf(got["blas_nodes"][:, :16].reshape(-1, 4, 4)[:, :, :3]).any()
    got, _ = moved(backend, got, swapped(1, 12), "a move over the bad records")
    back, d = refitted(backend, got, 0, i0, good, "a good refit after the bad one")
    backend.synchronize()
    assert (d["entry_lo"][:, 0] <= d["entry_hi"][:, 0]).all()
    used = back["blas_nodes"][:, 3:16:4].view(np.int32) >= 0
    assert np.isfinite(back["blas_nodes"][:, :16].reshape(-1, 4, 4)[:, :, :3][used]).all()
    assert backend.mesh_refit_info().bad_vertices == 4


def test_a_mesh_nobody_shows_is_left_alone(art, backend, options):
    options("inst_open", 1)
    A = placed(0)
    m = mats(A)
    sd = with_mats([0] * 12, m)
    ex = upload(backend, sd)
    assert ex["mesh_base"][1, 1] == -1 and ex["mesh_base"][0, 1] == 0
    shrunk = m.copy()
    shrunk.reshape(12, 3, 4)[:, :, :3] *= F(1.0e-2)                              # every pad would rise
    got, d = moved(backend, ex, shrunk, "a mesh without instances")
    assert d["repadded"] == [0] and got["mesh_pad"][1] == ex["mesh_pad"][1]
    at = np.nonzero(ex["node_mesh"] == 1)[0]
    qb = int(ex["mesh_base"][1, 2])
    assert np.array_equal(got["blas_nodes"][at].view(np.uint32), ex["blas_nodes"][at].view(np.uint32))
    assert np.array_equal(got["qnodes"][qb:qb + at.size], ex["qnodes"][qb:qb + at.size])
    assert np.array_equal(got["blas_tris"].view(np.uint32), ex["blas_tris"].view(np.uint32))
    p0, _, i0 = verts(sd, 0)
    refitted(backend, got, 0, i0, (p0 * F(1.5)).astype(F), "and a refit of the mesh that is shown")


# ---- d. behaviour at the shapes of b -------------------------------------------------------------------------------------------------
def aimed_rays(m, n, seed, spread):
    """n rays from around the camera towards the instances' origins (test_ray_queries_and_the_debug_pass_see_the_flattened_scene)"""
    rng = np.random.default_rng(seed)
    m = np.asarray(m, F).reshape(-1, 3, 4)
    o = np.tile(np.array([0.0, 2.55, 12.5], F), (n, 1)) + rng.normal(0, 0.05, (n, 3)).astype(F)
    centres = m[:, :, 3]
    d = (centres[rng.integers(0, centres.shape[0], n)] + rng.normal(0, spread, (n, 3)).astype(F) - o).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def behaviour_case(art, name):
    """(scene to upload, matrices to move to, the target scene, spread of the rays' aim)"""
    if name in ("65", "300"):
        n = int(name)
        m = swapped(1, n)
        return placed(0, n), m, with_mats(mesh_of(placed(0, n)), m), 0.2
    if name == "grid257":
        mesh = grid_mesh(art, 257)
        return custom(art, [mesh], [(0, _target(0))]), _target(1)[None], custom(art, [mesh], [(0, _target(1))]), 0.15
    meshes, m = awkward("awkward")
    return with_mats(meshes, mats(placed(0, len(meshes)))), m, with_mats(meshes, m), 0.25


@pytest.mark.parametrize("name", ["65", "300", "grid257", "awkward"])
def test_rays_after_a_move_equal_the_oracle_on_the_flattened_target(art, backend, options, name):
    options("inst_open", 0)
    start, m, target, spread = behaviour_case(art, name)
    flat = hostsim.flattened_copy(art, target)
    assert flat.desc.meshes[0].ntris <= 20000
    o, d = aimed_rays(m, 3000, 11, spread)
    w = conv.hits_to_arrays(orc.closest_hits(conv.OracleScene(flat).scene, o, d))
    on_mesh = (w[1] == 1) & (w[2] == 2)
    share = float(on_mesh.mean())
    print("oracle: %.1f %% of the rays hit a mesh triangle (%s)" % (100.0 * share, name))
    assert share >= 0.10                                                         # by the oracle alone, before anything runs on the GPU
    ntris = [target.desc.meshes[mi].ntris for mi in mesh_of(target)]
    offs = np.concatenate([[0], np.cumsum(ntris)])
    shift = int(np.ceil(np.log2(max(target.desc.meshes[k].ntris for k in range(target.desc.n_meshes)))))
    ex = upload(backend, start)
    moved(backend, ex, m, name)
    og, dg = gpu(o), gpu(d)
    for kernel in (art.TRACE_COOP, art.TRACE_SIMPLE):
        h = backend.trace_rays_torch(og, dg, kernel=kernel)
        raw = h.raw.cpu().numpy()
        hit = w[1] == 1
        assert np.array_equal(raw[:, 1], w[1]), "is_hit differs for %d rays" % int((raw[:, 1] != w[1]).sum())
        assert np.array_equal(raw[hit, 2], w[2][hit]) and np.array_equal(raw[hit, 5], w[4][hit])
        assert np.array_equal(raw[hit, 0].view(np.uint32), w[0][hit].view(np.uint32)), "t differs"
        assert np.array_equal(raw[hit, 6:9].view(np.uint32), w[5][hit].view(np.uint32)), "normal differs"
        prim = raw[:, 3].astype(np.int64)
        assert np.array_equal(offs[prim[on_mesh] >> shift] + (prim[on_mesh] & ((1 << shift) - 1)), w[3][on_mesh])
        assert np.array_equal(prim[hit & ~on_mesh], w[3][hit & ~on_mesh])
    occ = backend.occluded_torch(og, dg).cpu().numpy()
    assert np.array_equal(occ, w[1] == 1)


# ---- e. refusals ----------------------------------------------------------------------------------------------------------------------
def test_a_flat_scene_is_refused_and_an_export_changes_no_picture(art, backend, options):
    from ada_ray_tracer_amd import scenes
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=21)

    def render():
        backend.resize(64, 48)
        accum, _, _ = backend.render_pass(p, 0)
        return accum.view(np.uint32).copy(), backend.stats().rays
    backend.upload_scene(scenes.synthetic_scene(2000, 3))
    want = render()
    with pytest.raises(art.ArtError, match="art_export_two_level: the scene is not instanced.*art_export_bvh"):
        backend.export_two_level()
    got = render()
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    A = placed(0)
    backend.upload_scene(A)
    want = render()
    backend.export_two_level()
    backend.move_instances_torch(gpu(mats(A)))
    backend.export_two_level()
    got = render()
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    with pytest.raises(art.ArtError, match="only its sizes are reported"):
        backend.export_bvh()
    info = art.ArtTwoLevelInfo(); buf = art.ArtTwoLevelBuffers()
    tiny = np.zeros(4, F)
    buf.mesh_box = tiny.ctypes.data; buf.cap[7] = 4
    assert backend.lib.art_export_two_level(info, buf) != 0
    assert "buffer mesh_box too small" in backend.lib.art_last_error().decode()


SCRIPT = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import ctypes as C
out = {}
be = art.Backend(0)
L = be.lib
try:
    be.export_two_level()
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
    be.export_two_level()
    out["gcore"] = "accepted"
except art.ArtError as e:
    out["gcore"] = str(e)
h1 = art.HitCpp(); hit1 = bool(L.gcore_closest_hit(o, d, 0.0, 100.0, C.byref(h1)))
out["gcore_unchanged"] = bool(hit0 and hit0 == hit1 and h0.t == h1.t and h0.primIndex == h1.primIndex)
L.gcore_destroy()
be.shutdown()
print("RESULT " + json.dumps(out))
'''


def test_the_refusals_of_a_fresh_process(art):
    """no scene, and a scene committed through the gcore seam (a child process: the library is a process-wide singleton)"""
    r = subprocess.run([sys.executable, "-c", SCRIPT, art.ROOT], capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(line[0][7:])
    assert "art_export_two_level: no scene uploaded" in out["no_scene"]
    assert "gcore_commit_scene" in out["gcore"] and out["gcore_unchanged"]
