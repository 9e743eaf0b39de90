"""tests/two_level_ref.py against the host builder, without a GPU: tests/host_sim exports build_two_level_host's arrays (hs_two_level) in
the form of Backend.export_two_level(), and the reference update of one build must give what the builder gives for the target.  This is
what settles the reference before tests/test_gpu_two_level_reference.py holds the kernels to it.  Every comparison is exact."""
import numpy as np
import pytest

import hostsim
import refit_ref
import two_level_ref as ref

F = np.float32
SEED = 0xADA5EED0 + 64
TRIS = 40                        # the smallest meshes scenes.instanced_scene makes: a 7 x 3 torus (42 triangles) and a 4 x 4 grid (32)


def placed(k, n=12, tris=TRIS):
    from ada_ray_tracer_amd import scenes
    return scenes.instanced_scene(n, tris, seed=SEED + k)


def mats(sd):
    return np.array([list(sd.desc.instances[i].m) for i in range(sd.desc.n_instances)], F)


def planes(q):
    """a quantised node without its entry words (they are absolute: they count the instance tree's nodes in front)"""
    return np.ascontiguousarray(q.reshape(-1, 4, 4)[:, :, [0, 1, 3]])


@pytest.fixture
def inst_open(art):
    """option inst_open of the following host builds, put back to the default afterwards"""
    yield lambda v: hostsim.set_bvh_param(art, "inst_open", v)
    hostsim.set_bvh_param(art, "inst_open", 0)


def built(art, sd):
    ex = hostsim.two_level(art, sd)
    assert ex["updated"] == 0 and ex["n_inst"] == sd.desc.n_instances
    return ex


@pytest.mark.parametrize("n", [1, 12, 65])
@pytest.mark.parametrize("opened", [1, 8])
def test_a_move_to_the_uploaded_matrices_reproduces_the_build(art, inst_open, n, opened):
    inst_open(opened)
    sd = placed(0, n)
    ex = built(art, sd)
    if opened > 1:
        assert ex["inst"].shape[0] > n                                           # more entry points than instances
    got, d = ref.move(ex, mats(sd), details=True)
    assert d["ok"].all() and not d["repadded"]
    ref.assert_equal(got, ex, "%d instances, inst_open %d" % (n, opened))
    for mi in range(2):                                                          # and a refit of every node of the meshes' trees
        if ex["mesh_base"][mi, 1] < 0:                                           # (one instance: the grid is shown by nobody)
            assert n == 1 and mi == 1
            continue
        want_box = ex["mesh_box"][mi].copy()
        S = ref.copy_of(ex)
        tlo, thi = ref._refit_mesh_tree(S, mi, S["mesh_pad"][mi])
        ref.assert_equal(S, ex, "mesh %d refitted" % mi)
        assert np.array_equal(np.concatenate([tlo, thi]), want_box)


def test_a_mesh_refit_to_the_uploaded_vertices_reproduces_the_build(art, inst_open):
    inst_open(8)
    sd = placed(0, 12)
    ex = built(art, sd)
    for mi in range(2):
        pos, _, idx, _, _ = sd._mesh_arrays[mi]
        got, d = ref.refit_mesh(ex, mi, idx, pos, details=True)
        assert not d["repadded"]
        ref.assert_equal(got, ex, "mesh %d" % mi)


@pytest.mark.parametrize("n", [12, 65])
def test_a_move_from_a_to_b_matches_the_build_of_b(art, inst_open, n):
    """What a move shares with an upload at the new matrices: the instance table, every instance's box and proxy corners, the pads
    wherever B's is at least A's, and -- the meshes' trees do not depend on the matrices but through the pad -- the node packets and
    quantised nodes of every mesh whose pad after the move is B's.  (The instance tree's topology is A's: not comparable.)"""
    inst_open(1)
    A, B = placed(0, n), placed(1, n)
    ea, eb = built(art, A), built(art, B)
    got, d = ref.move(ea, mats(B), details=True)
    assert d["ok"].all()
    refit_ref.diff_report(got["inst"][:, :24], eb["inst"][:, :24], "m and minv")
    assert np.array_equal(got["inst"][:, 24:], ea["inst"][:, 24:])
    keep = [k for k in range(24, 32) if k != ref.QROOT]                          # (qroot counts the instance tree's nodes, and B's tree is another)
    assert np.array_equal(ea["inst"][:, keep], eb["inst"][:, keep])
    pa = got["tlas_tris"][np.argsort(got["tlas_tris"][:, 9].view(np.int32))]
    pb = eb["tlas_tris"][np.argsort(eb["tlas_tris"][:, 9].view(np.int32))]
    refit_ref.diff_report(pa, pb, "proxy records by instance")
    refit_ref.diff_report(np.concatenate([d["entry_lo"], d["entry_hi"]], 1), pb[:, :6], "entry boxes")
    compared = 0
    for mi in range(2):
        if eb["mesh_pad"][mi] >= ea["mesh_pad"][mi]:
            assert got["mesh_pad"][mi].view(np.uint32) == eb["mesh_pad"][mi].view(np.uint32), "pad of mesh %d" % mi
        else:
            assert got["mesh_pad"][mi] == ea["mesh_pad"][mi]                     # pads only grow
        if got["mesh_pad"][mi] == eb["mesh_pad"][mi]:
            nb, nn, tb, nrec, qb = ref.mesh_slices(got, mi)
            assert (nb, nn, tb, nrec) == ref.mesh_slices(eb, mi)[:4]
            qb_b = ref.mesh_slices(eb, mi)[4]
            refit_ref.diff_report(got["blas_nodes"][nb:nb + nn], eb["blas_nodes"][nb:nb + nn], "mesh %d: node" % mi)
            refit_ref.diff_report(planes(got["qnodes"][qb:qb + nn]), planes(eb["qnodes"][qb_b:qb_b + nn]), "mesh %d: quantised planes" % mi)
            compared += 1
    assert np.array_equal(got["blas_tris"], eb["blas_tris"]) and np.array_equal(got["mesh_box"], eb["mesh_box"])
    print("meshes compared:", compared, "repadded:", d["repadded"])


def test_a_move_that_raises_a_pad_matches_the_build_there(art, inst_open):
    """instance 0 shrunk to a speck: its mesh's pad rises to the build's value at the target, the other mesh keeps its own"""
    inst_open(1)
    A = placed(0, 12)
    m = mats(A)
    m[0].reshape(3, 4)[:, :3] *= F(1.0e-3)
    from ada_ray_tracer_amd import scenes
    B = scenes.instanced_scene(0, TRIS, transforms=[(int(A.desc.instances[i].mesh), m[i].reshape(3, 4)) for i in range(12)])
    ea, eb = built(art, A), built(art, B)
    got, d = ref.move(ea, m, details=True)
    assert d["repadded"] == [0]
    assert got["mesh_pad"][0] > ea["mesh_pad"][0] and got["mesh_pad"][1] == ea["mesh_pad"][1]
    refit_ref.diff_report(got["mesh_pad"], eb["mesh_pad"], "pads")
    refit_ref.diff_report(got["blas_nodes"], eb["blas_nodes"], "the meshes' nodes")
    refit_ref.diff_report(planes(got["qnodes"][ea["tlas_nodes"].shape[0]:]), planes(eb["qnodes"][eb["tlas_nodes"].shape[0]:]), "the meshes' quantised planes")


def test_bad_matrices_in_the_reference(art, inst_open):
    inst_open(1)
    A = placed(0, 12)
    ea = built(art, A)
    m = mats(A)
    m[3, 5] = np.nan; m[4] = 0.0; m[5, 3] = 2.0e18
    got, d = ref.move(ea, m, details=True)
    assert (~d["ok"]).nonzero()[0].tolist() == [3, 4, 5]
    assert not np.isfinite(d["entry_lo"][3:6]).any() and np.isfinite(d["entry_lo"][[0, 1, 2, 6]]).all()
    assert (got["inst"][3:5, 12:24] == 0).all() and (got["inst"][5, 12:24] != 0).any()      # (the far one has an inverse; its reach is what is bad)
    ids = got["tlas_tris"][:, 9].view(np.int32)
    assert np.array_equal(got["tlas_tris"][np.isin(ids, [3, 4, 5])], ea["tlas_tris"][np.isin(ids, [3, 4, 5])])      # the proxies keep their words
    assert np.isinf(got["tlas_nodes"]).any()
    back = ref.move(got, mats(A))
    ref.assert_equal(back, ea, "a good move after the bad one")
