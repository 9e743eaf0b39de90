"""art_refit_device against an independent refit (tests/refit_ref.py, plain numpy, itself checked against the host builder in
tests/test_refit_reference_host.py): the re-exported nodes and triangle records of a moved mesh word for word, the trace kernels' own
copies (quantised nodes, padded records) through the traversal counters, hits against the brute-force oracle of the moved mesh, defined
answers while bad vertices empty some boxes, and the shapes the other refit tests do not reach.  Every comparison is exact."""
import numpy as np
import pytest

import bvh_check
import conv
import orc
import refit_ref
from test_gpu_parity import _assert_hits_equal, _random_rays
from test_gpu_refit import _deform, _export, _gpu, _mesh, _moved, _rays, _refit, _scene
from test_refit_reference_host import MAY_MISS, SHAPES, _shift, mesh_scene, rays_at, shape_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
KERNELS = ("TRACE_COOP", "TRACE_SIMPLE")


@pytest.fixture
def options(backend):
    """Options set by a test are put back to the defaults afterwards (the session's backend is shared)."""
    yield backend.set_option
    for name, value in (("bvh_width", 4), ("bvh_builder", 3), ("bvh_spatial_splits", 0)):
        backend.set_option(name, value)


def _expect_tree(backend, n0, t0, width, idx, pos, what):
    """The re-exported tree equals the reference refit of (n0, t0) to pos; returns the exported (nodes, tris, info)."""
    want_nodes, want_tris = refit_ref.refit(n0.view(F), t0.view(F), width, idx, pos)
    n1, t1, info = _export(backend)
    assert info.node_width == width
    refit_ref.diff_report(t1, want_tris, "%s: triangle record" % what)
    refit_ref.diff_report(n1, want_nodes, "%s: node" % what)
    return n1, t1, info


# ---- 1. moved mesh, word for word -----------------------------------------------------------------------------------------------------
MATRIX = [(name, b, w, 0) for name in ("structured", "synthetic") for b in (3, 0, 1, 2) for w in (4, 8)] + [("structured", 0, 4, 1), ("structured", 0, 8, 1)]


@pytest.mark.parametrize("name,builder,width,splits", MATRIX)
def test_moved_refit_equals_the_reference_word_for_word(art, backend, options, name, builder, width, splits):
    sd = _scene(name)
    options("bvh_width", width); options("bvh_builder", builder); options("bvh_spatial_splits", splits)
    backend.upload_scene(sd)
    n0, t0, i0 = _export(backend)
    pos, nrm, idx, _ = _mesh(sd)
    if splits:
        assert i0.n_tris > idx.shape[0]                                           # several records per primitive
    p2, n2 = _deform(name, pos, nrm, amount=2.0)
    _refit(backend, p2, n2)
    _expect_tree(backend, n0, t0, width, idx, p2, "first refit")
    p3, n3 = _deform(name, p2, n2, seed=4, amount=-0.7)                           # on top of it: the scratch holds an earlier refit's tight boxes
    assert not np.array_equal(p3, p2) and not np.array_equal(p3, pos)
    _refit(backend, p3, n3)
    _expect_tree(backend, n0, t0, width, idx, p3, "second refit")
    ri = backend.refit_info()
    assert ri.refits == 2 and ri.bad_vertices == 0


# ---- 2. the kernels' own copies agree with the exported tree ------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
def test_counters_after_a_refit_match_the_walk_of_the_reexported_tree(art, backend, options, width):
    """TRACE_COOP at width 4 reads only the quantised nodes and the padded records: equal t bits, primitives and counters tie those to the
    binary32 tree art_export_bvh returns (which item 1 ties to the reference)."""
    from ada_ray_tracer_amd import scenes
    mesh = scenes.random_triangles(20000, 77)
    lights = [dict(shape=art.LIGHT_SPHERE, mat=4, center=(0.0, 4.5, 1.0), radius=0.5, intensity=(10.0, 10.0, 10.0), surfaceArea=3.14159)]
    sd = art.SceneDesc([], lights, scenes.cornell_materials(), [mesh], None, scenes.REFERENCE_CAMERA)   # mesh only: every ray starts unbounded
    options("bvh_width", width)
    backend.upload_scene(sd)
    n0, t0, _ = _export(backend)
    o, d = _random_rays(40000, 8)
    d[:100, 0] = 0.0                                                              # axis-parallel directions
    d[100:200, 1] = 0.0; d[200:230, :2] = 0.0; d[200:230, 2] = 1.0
    _, before = backend.trace_rays(o, d, want_stats=True)
    new = _shift(mesh["pos"], 21)
    _refit(backend, new)
    n1, t1, info = _expect_tree(backend, n0, t0, width, mesh["idx"], new, "moved soup")
    t, prim, cnt = orc.bvh_walk(n1.view(F), t1.view(F), o, d, width=info.node_width)
    assert (prim >= 0).sum() > 5000
    for kernel in KERNELS:
        hits, st = backend.trace_rays(o, d, kernel=getattr(art, kernel), want_stats=True)
        gprim = np.array([h.prim_index if h.is_hit else -1 for h in hits], np.int32)
        gt = np.array([h.t for h in hits], np.float32)
        assert np.array_equal(gprim, prim), "%s: %d primitives differ" % (kernel, int((gprim != prim).sum()))
        assert np.array_equal(gt[prim >= 0].view(np.uint32), t[prim >= 0].view(np.uint32)), kernel
        assert (st.box_tests, st.tri_tests, st.node_visits, st.leaf_visits, st.traced_rays) == \
               (cnt.box_tests, cnt.tri_tests, cnt.node_visits, cnt.leaf_visits, cnt.rays), kernel
    assert (before.box_tests, before.tri_tests) != (cnt.box_tests, cnt.tri_tests)  # the move shows in the counters


# ---- 3. hits against the brute-force oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder,width,splits", [(3, 4, 0), (0, 8, 0), (0, 4, 1)])
def test_hits_after_a_refit_equal_the_brute_force_oracle(art, backend, options, builder, width, splits):
    sd = _scene("structured")
    options("bvh_width", width); options("bvh_builder", builder); options("bvh_spatial_splits", splits)
    backend.upload_scene(sd)
    pos, nrm, idx, _ = _mesh(sd)
    p2, n2 = _deform("structured", pos, nrm, amount=2.0)
    _refit(backend, p2, n2)
    o, d = _rays(12000, 7)
    want = orc.closest_hits(conv.OracleScene(_moved(art, sd, p2, n2)).scene, o, d)
    w = conv.hits_to_arrays(want)
    assert ((w[1] == 1) & (w[2] == 2)).sum() > 500                                # (prim_type 2: the moved mesh is actually hit)
    for kernel in KERNELS:
        _assert_hits_equal(backend.trace_rays(o, d, kernel=getattr(art, kernel)), want)


# ---- 4. bad vertices have defined answers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("name", ["structured", "synthetic"])
def test_bad_vertices_leave_the_brute_force_answer_over_the_surviving_records(art, backend, options, name, width):
    """structured: shared vertices, fewer vertices than records; synthetic: a soup, three vertices per record -- bad vertices whose index
    lies above the record count must be counted too."""
    sd0 = _scene(name)
    pos, nrm, idx, matid = _mesh(sd0)
    pos = np.concatenate([pos, np.array([[0.5, 2.0, 2.0]], F)]); nrm = np.concatenate([nrm, np.array([[0.0, 1.0, 0.0]], F)])   # + a vertex no triangle uses
    extra = pos.shape[0] - 1
    assert not (idx == extra).any()

    def scene(p, n, tri_idx, tri_mat):
        return art.SceneDesc(meshes=[dict(mode=art.MESH_CLOSEST, pos=p, nrm=n, idx=tri_idx, matid=tri_mat)], **sd0._kw)

    options("bvh_width", width)
    backend.upload_scene(scene(pos, nrm, idx, matid))
    n0, t0, _ = _export(backend)
    p2, n2 = _deform(name, pos, nrm)
    nt = idx.shape[0]
    victims = [7, nt * 3 // 20, nt * 9 // 20, nt * 3 // 4, nt - 1]                # (structured: triangles of the torus and of the grid)
    bad = p2.copy()
    for k, (tri, corner, axis, value) in enumerate(zip(victims, (0, 1, 2, 0, 1), (1, 0, 2, 0, 2), (np.nan, np.inf, F(3e18), -np.inf, F(-3e18)))):
        bad[idx[tri, corner], axis] = value
    bad[idx[victims[0], 0], 2] = np.nan                                           # (two bad coordinates of one vertex: one bad vertex)
    bad[extra, 1] = np.inf
    bad_verts = np.nonzero(~(np.abs(bad) <= 1e18).all(axis=1))[0]
    assert bad_verts.size == 6
    using = np.isin(idx, bad_verts).any(axis=1)                                   # triangles that use a bad vertex (the vertices are shared)
    assert using[victims].all() and 5 <= using.sum() <= 60

    backend.refit_torch(_gpu(bad)[0], _gpu(n2)[0], check=False)
    torch.cuda.synchronize()
    with pytest.raises(art.ArtError, match="6 vertex coordinate"):
        backend.synchronize()
    assert backend.refit_info().bad_vertices == 6
    n1, t1, info = _expect_tree(backend, n0, t0, width, idx, bad, "refit with bad vertices")

    alive = refit_ref.surviving_records(n1.view(F), t1.view(F), width)
    prim = t1.reshape(-1, 12)[:, 9].view(np.int32)
    survivors = np.unique(prim[alive])
    lost = np.setdiff1d(np.arange(idx.shape[0]), survivors)
    assert using[lost].any() and np.isin(np.nonzero(using)[0], lost).all(), "a triangle with a bad vertex survived"
    assert (~alive).sum() <= refit_ref.MAX_LEAF_TRIS * int(using.sum()), "%d records lost for %d triangles with a bad vertex" % ((~alive).sum(), using.sum())
    assert np.isin(prim[~alive], lost).all()                                      # (no primitive is half lost)

    clean = np.where((np.abs(bad) <= 1e18), bad, F(0.0)).astype(F)                # (the survivors use none of the replaced coordinates)
    assert np.array_equal(clean[idx[survivors]], bad[idx[survivors]])
    osc = conv.OracleScene(scene(clean, n2, np.ascontiguousarray(idx[survivors]), np.ascontiguousarray(matid[survivors])))
    o, d = _rays(16000, 13)
    centre = p2[idx[lost]].astype(np.float64).mean(axis=1)                        # + rays aimed at where the lost triangles would be
    rng = np.random.default_rng(5)
    aim = centre[rng.integers(0, centre.shape[0], 4000)] + 0.02 * rng.standard_normal((4000, 3))
    o2 = (rng.random((4000, 3)) * [4.6, 4.4, 4.6] + [-2.3, 0.3, 0.2])
    d2 = aim - o2; d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    o = np.ascontiguousarray(np.concatenate([o, o2.astype(F)])); d = np.ascontiguousarray(np.concatenate([d, d2.astype(F)]))
    want = orc.closest_hits(osc.scene, o, d)
    for h in want:
        if h.is_hit and h.prim_type == 2:
            h.prim_index = int(survivors[h.prim_index])                           # back to the uploaded mesh's numbering (monotone: ties keep their order)
    w = conv.hits_to_arrays(want)
    assert ((w[1] == 1) & (w[2] == 2)).sum() > 2000
    full = conv.hits_to_arrays(orc.closest_hits(conv.OracleScene(scene(clean, n2, idx, matid)).scene, o, d))
    assert (full[3] != w[3]).sum() > 100                                          # the rays do see the holes
    for kernel in KERNELS:
        _assert_hits_equal(backend.trace_rays(o, d, kernel=getattr(art, kernel)), want)
    og, dg = _gpu(o, d)
    occ = backend.occluded_torch(og, dg).cpu().numpy()
    assert np.array_equal(occ, w[1] == 1), "occlusion differs for %d rays" % int((occ != (w[1] == 1)).sum())

    _refit(backend, p2, n2)                                                       # a good refit: the whole tree again
    backend.synchronize()
    _expect_tree(backend, n0, t0, width, idx, p2, "good refit after the bad one")
    want = orc.closest_hits(conv.OracleScene(scene(p2, n2, idx, matid)).scene, o, d)
    for kernel in KERNELS:
        _assert_hits_equal(backend.trace_rays(o, d, kernel=getattr(art, kernel)), want)


# ---- 5. shapes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("name", SHAPES)
def test_shapes(art, backend, options, name, width):
    """The cases (tests/test_refit_reference_host.py shape_case; each also runs there on the CPU with a host-built tree):
      tri1, tri2            one and two triangles (the root holds one leaf; the host builder takes over below 2 triangles)
      soup255 .. soup513    record counts around the 256-lane block, three vertices per record (nverts > n_recs)
      grid255 .. grid513    the same counts with shared vertices (nverts < n_recs)
      unreferenced          300 triangles and 1 000 trailing vertices no triangle uses
      point, plane_y        every vertex at one point / every y at one value: zero extents through the padding and the 8-bit grid
      scale_1e-30, 1e9, 9e17  the largest coordinate magnitude; 9e17 lies just inside the refit's limit of 1e18
      neg_zero              coordinates of -0.0 next to +0.0 in the same triangles
    In all of them, at both widths: the re-exported tree equals the reference word for word, check_tree's strict enclosure holds (the pad
    is never 0), no bad vertex is counted and both kernels return the oracle's hits (at 9e17: is_hit and the primitive; nothing is hit
    there, at 1e-30 or on the point, see MAY_MISS).  Axis-parallel rays are part of every case below 3e8 (rays_at says why)."""
    pos, idx, new = shape_case(name)
    options("bvh_width", width)
    backend.upload_scene(mesh_scene(art, pos, idx))
    n0, t0, i0 = _export(backend)
    assert i0.n_tris == idx.shape[0]
    _refit(backend, new)
    backend.synchronize()
    assert backend.refit_info().bad_vertices == 0
    n1, t1, info = _expect_tree(backend, n0, t0, width, idx, new, name)
    bvh_check.check_tree(n1.view(F), t1.view(F), info.n_nodes, info.max_stack, width, new, idx)
    o, d = rays_at(new, idx, 4000, 17)
    want = orc.closest_hits(conv.OracleScene(mesh_scene(art, new, idx)).scene, o, d)
    w = conv.hits_to_arrays(want)
    if name not in MAY_MISS:
        assert (w[1] == 1).mean() >= 0.25, "only %d of %d rays hit" % ((w[1] == 1).sum(), w[1].size)
    for kernel in KERNELS:
        got = backend.trace_rays(o, d, kernel=getattr(art, kernel))
        if name == "scale_9e17":                                                  # the binary32 triangle test overflows there: is_hit and the primitive
            g = conv.hits_to_arrays(got)
            assert np.array_equal(g[1], w[1]), "%s: is_hit differs for %d rays" % (kernel, int((g[1] != w[1]).sum()))
            assert np.array_equal(g[3][w[1] == 1], w[3][w[1] == 1]), kernel
        else:
            _assert_hits_equal(got, want)
