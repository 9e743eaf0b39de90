"""The builder options an upload and a rebuild promise to follow (include/art_hip.h art_rebuild_device):
bvh_max_leaf, the cost options bvh_leaf_base_milli / bvh_tri_cost_milli / bvh_node_cost_milli, and bvh_ploc_radius.  The GPU builders
clamp and default these on their own side (art_sah.hip, art_lbvh.hip), apart from the host builder (art_bvh.cpp): under every setting
the GPU SAH builder (3) must give the host builder's (0) tree -- the numbering-independent fingerprint of tests/tree_sig.py, node and
record counts, stack bound --, every builder's tree must be sound (tests/bvh_check.py), no leaf may hold more than min(max_leaf, width)
records, and 4000 rays must find the closest hits of the oracle's scan over all triangles, bit for bit."""
import numpy as np
import pytest

import bvh_check
import conv
import orc
from test_gpu_parity import _assert_hits_equal, _random_rays
from tree_sig import tree_signature

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")         # (imported before the backend opens the GPU, as in tests/test_gpu_rebuild.py: the rebuild takes torch tensors)

SCENES = ("soup-9", "soup-2049", "soup-3000", "grid-16")         # 2049: one reference more than the SAH builder's 2048-reference chunk
DEFAULTS = (("bvh_width", 4), ("bvh_builder", 3), ("bvh_max_leaf", 0), ("bvh_leaf_base_milli", 1000), ("bvh_tri_cost_milli", -1000),
            ("bvh_node_cost_milli", 400), ("bvh_ploc_radius", 8))
# Each cost option alone at 0 and at 1500, one combination of all three, and a negative bvh_tri_cost_milli (= the width's default cost)
COST_SETTINGS = [{"bvh_leaf_base_milli": 0}, {"bvh_leaf_base_milli": 1500}, {"bvh_tri_cost_milli": 0}, {"bvh_tri_cost_milli": 1500},
                 {"bvh_node_cost_milli": 0}, {"bvh_node_cost_milli": 1500},
                 {"bvh_leaf_base_milli": 500, "bvh_tri_cost_milli": 300, "bvh_node_cost_milli": 1200}, {"bvh_tri_cost_milli": -1}]


@pytest.fixture
def options(backend):
    """Options set by a test are put back to the defaults afterwards (the session's backend is shared)."""
    yield backend.set_option
    for name, value in DEFAULTS:
        backend.set_option(name, value)


_cache = {}


def case(art, name):
    """(scene, mesh positions, mesh indices, 4000 rays and the oracle's closest hits of them): once per scene"""
    if name not in _cache:
        from ada_ray_tracer_amd import scenes
        if name.startswith("soup"):
            sd = scenes.synthetic_scene(int(name.split("-")[1]), 3)
        else:
            lights = [dict(shape=art.LIGHT_SPHERE, mat=4, center=(0.0, 4.5, 1.0), radius=0.5, intensity=(10.0, 10.0, 10.0), surfaceArea=3.14159)]
            sd = art.SceneDesc([], lights, scenes.cornell_materials(), [scenes.grid_mesh(16)], None, scenes.REFERENCE_CAMERA)
        pos, _, idx, _, _ = sd._mesh_arrays[-1]
        o, d = _random_rays(4000, 41)
        _cache[name] = (sd, pos, idx, o, d, orc.closest_hits(conv.OracleScene(sd).scene, o, d))
    return _cache[name]


def leaf_counts(nodes, width):
    """record counts of the leaf slots of an exported tree (layout: csrc/art_scene.h)"""
    nd = np.asarray(nodes, np.float32).reshape(-1, 8 * width)
    ref = nd[:, 3:4 * width:4].view(np.int32); cnt = nd[:, 4 * width + 3:8 * width:4].view(np.int32)
    return cnt[(ref >= 0) & (cnt > 0)]


def upload(backend, name_case, builder):
    """upload under `builder`; (fingerprint, n_nodes, n_tris, max_stack) and the export"""
    backend.set_option("bvh_builder", builder)
    backend.upload_scene(name_case[0])
    nodes, tris, info = backend.export_bvh()
    return (tree_signature(nodes, tris, info), info.n_nodes, info.n_tris, info.max_stack), (nodes, tris, info)


def sound_and_hits(backend, name_case, export, width, leaf_bound):
    """the uploaded tree is sound, keeps the leaf bound, and the trace kernel finds the oracle's hits through it"""
    sd, pos, idx, o, d, want = name_case
    nodes, tris, info = export
    assert info.node_width == width
    rep = bvh_check.check_tree(nodes, tris, info.n_nodes, info.max_stack, width, pos, idx)
    assert rep["records"] == idx.shape[0]
    lc = leaf_counts(nodes, width)
    assert lc.size > 0 and lc.max() <= leaf_bound, "a leaf of %d records under a bound of %d" % (lc.max(), leaf_bound)
    _assert_hits_equal(backend.trace_rays(o, d), want)
    return lc


@pytest.mark.parametrize("max_leaf", range(1, 9))
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("scene", SCENES)
def test_max_leaf_gpu_sah_builds_the_host_builders_tree(art, backend, options, scene, width, max_leaf):
    c = case(art, scene)
    options("bvh_width", width); options("bvh_max_leaf", max_leaf)
    host, _ = upload(backend, c, 0)
    gpu, export = upload(backend, c, 3)
    assert gpu == host, "host %s, GPU %s" % (host, gpu)
    lc = sound_and_hits(backend, c, export, width, min(max_leaf, width))
    print("%s width %d max_leaf %d: %d nodes, %d leaves, largest %d" % (scene, width, max_leaf, gpu[1], lc.size, lc.max()))


@pytest.mark.parametrize("max_leaf", range(1, 9))
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("builder", [1, 2], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("scene", SCENES)
def test_max_leaf_lbvh_and_ploc(art, backend, options, scene, builder, width, max_leaf):
    c = case(art, scene)
    options("bvh_width", width); options("bvh_max_leaf", max_leaf)
    _, export = upload(backend, c, builder)
    sound_and_hits(backend, c, export, width, min(max_leaf, width))


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("scene", SCENES)
def test_cost_options(art, backend, options, scene, width):
    """Every setting: the GPU SAH tree is the host's, sound, within the default leaf bound, and finds the oracle's hits.  A negative
    bvh_tri_cost_milli gives the width's default tree, and at least two settings give another tree than the defaults (an option that
    is ignored on both sides would otherwise pass).

    bvh_tri_cost_milli = 0 on the two larger soups is the case that reaches the builders' fallback: with no cost per triangle the SAH
    has no reason to balance, the binary tree grows deeper than max_sah_depth (48), and below that depth a node is cut into the first
    count / 2 references by (centroid on the widest axis, triangle id) -- on both sides (art_bvh.cpp's nth_element, art_sah.hip's
    pos_key).  Until art_sah.hip did the same it cut its current reference order there: 713 nodes against the host's 626 for
    soup-2049 at width 4."""
    c = case(art, scene)
    options("bvh_width", width)
    default, _ = upload(backend, c, 3)
    different, mismatch = [], []
    for setting in COST_SETTINGS:
        for name, value in DEFAULTS[3:6]:
            options(name, setting.get(name, value))
        host, _ = upload(backend, c, 0)
        gpu, export = upload(backend, c, 3)
        print("%s width %d %s: host %s, GPU %s" % (scene, width, setting, host[1:], gpu[1:]))
        if gpu != host:
            mismatch.append((setting, host, gpu))
        sound_and_hits(backend, c, export, width, width)
        if setting == {"bvh_tri_cost_milli": -1}:
            assert gpu == default
        elif gpu != default:
            different.append(setting)
    print("%s width %d: trees other than the default one under %s" % (scene, width, different))
    assert len(different) >= 2
    assert not mismatch, "the GPU SAH tree is not the host builder's under %s" % (mismatch,)


@pytest.mark.parametrize("radius", [1, 64])
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("scene", ["soup-9", "soup-3000"])          # 9: fewer clusters than the radius
def test_ploc_radius(art, backend, options, scene, width, radius):
    c = case(art, scene)
    options("bvh_width", width); options("bvh_ploc_radius", radius)
    _, export = upload(backend, c, 2)
    sound_and_hits(backend, c, export, width, min(1 if width == 4 else 2, width))      # (bvh_max_leaf = 0: the GPU builders' own leaf size)


@pytest.mark.parametrize("width", [4, 8])
def test_rebuild_follows_the_builder_options_as_they_stand(art, backend, options, width):
    """Uploaded at the defaults, rebuilt after bvh_max_leaf = 2 and bvh_node_cost_milli = 1500 were set: word for word the export of an
    upload made under those options (the pattern of test_gpu_rebuild.test_rebuild_follows_the_options_as_they_stand)."""
    import test_gpu_refit as T
    sd = T._scene("synthetic")
    pos, nrm, idx, _ = T._mesh(sd)
    p2, n2 = T._deform("synthetic", pos, nrm)
    moved = T._moved(art, sd, p2, n2)
    options("bvh_width", width); options("bvh_builder", 3)
    backend.upload_scene(moved)
    plain = T._export(backend)
    options("bvh_max_leaf", 2); options("bvh_node_cost_milli", 1500)
    backend.upload_scene(moved)
    want = T._export(backend)
    assert not np.array_equal(plain[0], want[0])                         # the options change the tree
    options("bvh_max_leaf", 0); options("bvh_node_cost_milli", 400)
    backend.upload_scene(sd)
    options("bvh_max_leaf", 2); options("bvh_node_cost_milli", 1500)
    pg, ng = T._gpu(p2, n2)
    backend.rebuild_torch(pg, ng)
    got = T._export(backend)
    assert (got[2].n_nodes, got[2].n_tris, got[2].max_stack, got[2].node_width) == (want[2].n_nodes, want[2].n_tris, want[2].max_stack, width)
    assert np.array_equal(got[1], want[1]), "triangle records differ"
    assert np.array_equal(got[0], want[0]), "%d of %d node words differ" % (int((got[0] != want[0]).sum()), want[0].size)
    assert leaf_counts(got[0].view(np.float32), width).max() <= 2
    bvh_check.check_tree(got[0].view(np.float32), got[1].view(np.float32), got[2].n_nodes, got[2].max_stack, width, p2, idx)
