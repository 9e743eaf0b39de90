"""The cooperative trace kernel's live-ray queue cut into 1, 2, 4 and 8 segments (option queue_segments: the segment bounds, one cursor
per segment, and a wave that has drained its own segment helping with the next) and its grid sized by option blocks_per_cu (0: the
occupancy query; n: n workgroups per CU).  Neither may change a hit, a picture, a ray count or a traversal counter: every comparison is
with the CPU oracle and exact."""
import numpy as np
import pytest

import conv
import hostsim
import orc
from test_gpu_parity import _assert_hits_equal, _random_rays, bits

pytestmark = pytest.mark.gpu

# (queue_segments, blocks_per_cu): every segment count at the occupancy default and at one workgroup per CU, two per CU at 8 segments
COMBOS = [(s, b) for s in (1, 2, 4, 8) for b in (0, 1)] + [(8, 2)]
COMBO_IDS = ["seg%d-bpc%d" % c for c in COMBOS]
# 1 .. 9 rays: zero or one ray in a segment, and one workgroup that walks every segment; 4097: beyond k_analytic's 4096-ray chunk
N_RAYS = (1, 3, 8, 9, 100, 4097)
W, H, DEPTH, SEED = 23, 11, 4, 17


@pytest.fixture(params=COMBOS, ids=COMBO_IDS)
def queue(backend, request):
    """the backend with one (queue_segments, blocks_per_cu) pair set; everything a test of this file sets is put back afterwards"""
    backend.set_option("queue_segments", request.param[0])
    backend.set_option("blocks_per_cu", request.param[1])
    yield backend
    for name, value in (("queue_segments", 8), ("blocks_per_cu", 0), ("bvh_width", 4), ("lds_stack_cap", 0), ("inst_coop", 1), ("count_tests", 0)):
        backend.set_option(name, value)


_cache = {}


def soup(art):
    """synthetic_scene(300, 3), its oracle scene, 4097 rays and the oracle's closest hits of them (computed once; a prefix of the rays
    has a prefix of the hits)"""
    if "soup" not in _cache:
        from ada_ray_tracer_amd import scenes
        sd = scenes.synthetic_scene(300, 3)
        osc = conv.OracleScene(sd)
        o, d = _random_rays(max(N_RAYS), 301)
        d[:3, 0] = 0.0                                         # (axis-parallel: 1/0 in the slab test, also among the first rays)
        _cache["soup"] = (sd, osc, o, d, orc.closest_hits(osc.scene, o, d))
    return _cache["soup"]


def oracle_picture(art, name):
    """the oracle's 23x11 PT_MIS depth-4 frame of mixed_scene(1500, 5) / of the flattened instanced_scene(12, 300): once per scene"""
    if name not in _cache:
        from ada_ray_tracer_amd import scenes
        sd = scenes.mixed_scene(1500, 5) if name == "mixed" else scenes.instanced_scene(12, 300)
        flat = hostsim.flattened_copy(art, sd) if name == "instanced" else sd
        ref, spp, cnt = orc.render(conv.OracleScene(flat).scene, orc.make_params(W, H, orc.PT_MIS, True, DEPTH, 1, seed=SEED))
        _cache[name] = (sd, bits(ref).copy(), spp, cnt.rays)
    return _cache[name]


@pytest.mark.parametrize("width", [4, 8])
def test_closest_hits(art, queue, width):
    """art_trace_rays: k_analytic fills the queue and its count (queue_count), k_trace_coop reads both"""
    sd, osc, o, d, want = soup(art)
    queue.set_option("bvh_width", width)
    queue.upload_scene(sd)
    for n in N_RAYS:
        _assert_hits_equal(queue.trace_rays(o[:n], d[:n]), want[:n])
    assert sum(1 for h in want[:9] if h.is_hit) > 0 and sum(1 for h in want if h.prim_type == 2) > 100      # (prim_type 2: the mesh behind the tree is hit)


@pytest.mark.parametrize("width", [4, 8])
def test_closest_hits_through_the_overflow_queue(art, queue, width):
    """lds_stack_cap = 3: rays whose stack does not fit are queued for k_trace_overflow"""
    sd, osc, o, d, want = soup(art)
    queue.set_option("bvh_width", width)
    queue.set_option("lds_stack_cap", 3)
    queue.upload_scene(sd)
    assert queue.bvh_info().max_stack > 3                      # the cap is below the tree's bound: the checked-push kernel runs
    for n in (9, 4097):
        _assert_hits_equal(queue.trace_rays(o[:n], d[:n]), want[:n])


def _render(art, be, sd):
    be.upload_scene(sd)
    be.resize(W, H)
    accum, _, spp = be.render_pass(art.Backend.pass_params(art.PT_MIS, True, DEPTH, 1, seed=SEED), 0)
    st = be.stats()
    return bits(accum), spp, st.rays, st.lost_paths


def test_render_on_the_record_queue(art, queue):
    """a render pass: the queue is the stage's record array, its length items * mul read on the device"""
    sd, acc, spp, rays = oracle_picture(art, "mixed")
    got = _render(art, queue, sd)
    assert got[1:] == (spp, rays, 0)
    assert np.array_equal(got[0], acc)


@pytest.mark.parametrize("inst_coop", [1, 0])
def test_render_of_an_instanced_scene(art, queue, inst_coop):
    """inst_coop = 1: k_trace_coop<.., INST>; 0: k_trace_inst, one ray per lane, over the same records"""
    sd, acc, spp, rays = oracle_picture(art, "instanced")
    queue.set_option("inst_coop", inst_coop)
    got = _render(art, queue, sd)
    assert got[1:] == (spp, rays, 0)
    assert np.array_equal(got[0], acc)


@pytest.mark.parametrize("segments", [1, 2, 4, 8])
def test_counters_match_the_oracles_walk(art, backend, segments):
    """count_tests = 1, as test_gpu_widths.test_counters_match_oracle_walk: the kernel's box tests, triangle tests, node and leaf visits
    and traced rays equal the oracle's walk of the exported tree, however the queue is cut"""
    from ada_ray_tracer_amd import scenes
    mesh = scenes.random_triangles(3000, 77)
    lights = [dict(shape=art.LIGHT_SPHERE, mat=4, center=(0.0, 4.5, 1.0), radius=0.5, intensity=(10.0, 10.0, 10.0), surfaceArea=3.14159)]
    sd = art.SceneDesc([], lights, scenes.cornell_materials(), [mesh], None, scenes.REFERENCE_CAMERA)   # mesh only: every ray starts unbounded
    backend.set_option("queue_segments", segments)
    backend.set_option("count_tests", 1)
    try:
        backend.upload_scene(sd)
        nodes, tris, info = backend.export_bvh()
        o, d = _random_rays(4097, 8)
        d[:100, 0] = 0.0
        t, prim, cnt = orc.bvh_walk(nodes, tris, o, d, width=info.node_width)
        hits, st = backend.trace_rays(o, d, want_stats=True)
    finally:
        backend.set_option("queue_segments", 8)
        backend.set_option("count_tests", 0)
    gprim = np.array([h.prim_index if h.is_hit else -1 for h in hits], np.int32)
    gt = np.array([h.t for h in hits], np.float32)
    assert np.array_equal(gprim, prim) and (prim >= 0).sum() > 500
    assert np.array_equal(gt[prim >= 0].view(np.uint32), t[prim >= 0].view(np.uint32))
    assert (st.box_tests, st.tri_tests, st.node_visits, st.leaf_visits, st.traced_rays) == \
           (cnt.box_tests, cnt.tri_tests, cnt.node_visits, cnt.leaf_visits, cnt.rays)
