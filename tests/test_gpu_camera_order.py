"""Option camera_order: 1 = bounce 0 of the compacted schedule visits a batch's path slots tile-major (all samples of a 1024-pixel block
before the next block, csrc/art_camera_order.h), 0 = in slot order.  Slots keep their numbers and survivors are placed by atomics, so only
the ORDER of the items in the banks changes, which carries no meaning: everything a caller can see must be the same under both -- the
accum bits, the LDR frame, ArtStats::rays, the items every bounce read and kept, lost_paths == 0 -- and the counting variant must count
the same tests.  The default is 1, so the rest of the suite runs tile-major; this file keeps slot order covered.

The frame is 48x40 = 1920 pixels: a partial last unit (1920 = 7 * 256 + 128) and a partial last block (1920 = 1024 + 896)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, DEPTH = 48, 40, 3
DEFAULT_BATCH_PATHS = 128 << 20
COUNTERS = ("box_tests", "tri_tests", "node_visits")
DEFAULT_ORDER = 1          # the library's default (Options::camera_order): put back after every comparison, the rest of the suite runs on it


@pytest.fixture(scope="module")
def scene(art):
    from ada_ray_tracer_amd import scenes
    return scenes.synthetic_scene(2000, 3)


def render(art, be, order, aa=True, vthreads=2, width=W, height=H, rt=None):
    be.set_option("camera_order", order)
    be.resize(width, height)
    s0, g0 = be.stats(), be.stage_stats()
    in0, out0 = list(g0.items_in), list(g0.items_out)
    accum, screen, spp = be.render_pass(art.Backend.pass_params(art.PT_MIS if rt is None else rt, aa, DEPTH, vthreads, seed=5), 0, want_screen=True)
    st, g1 = be.stats(), be.stage_stats()
    assert st.lost_paths == 0                                  # no path is lost
    items_in = [a - b for a, b in zip(g1.items_in, in0)]
    items_out = [a - b for a, b in zip(g1.items_out, out0)]
    assert items_in[0] == (st.samples - s0.samples) > 0        # bounce 0 read every slot once
    return dict(accum=np.ascontiguousarray(accum).view(np.uint32).copy(), screen=np.array(screen, copy=True), spp=spp, rays=st.rays - s0.rays,
                items_in=items_in, items_out=items_out, batches=g1.batches - g0.batches,
                counters=tuple(getattr(st, k) - getattr(s0, k) for k in COUNTERS))


def both(art, be, **kw):
    try:
        slot_order = render(art, be, 0, **kw)
        tile_major = render(art, be, 1, **kw)
    finally:
        be.set_option("camera_order", DEFAULT_ORDER)
    a, b = tile_major, slot_order
    assert a["spp"] == b["spp"] and a["batches"] == b["batches"]
    assert np.array_equal(a["accum"], b["accum"])
    assert np.array_equal(a["screen"], b["screen"])
    assert a["rays"] == b["rays"] > 0
    assert a["items_in"] == b["items_in"] and a["items_out"] == b["items_out"] and a["items_out"][0] > 0
    return a, b


@pytest.mark.parametrize("shade_per", [2, 4])
def test_one_batch_partial_unit_and_block(art, backend, scene, shade_per):
    """pn = 1920, sn = 8: 8 units per sample row, the last of 128 slots; block 1 has 896 pixels"""
    backend.upload_scene(scene)
    backend.set_option("shade_per", shade_per)
    try:
        a, _ = both(art, backend)
    finally:
        backend.set_option("shade_per", 0)
    assert a["spp"] == 8 and a["batches"] == 1 and a["items_in"][0] == 8 * W * H


def test_small_batches_pixels_first(art, backend, scene):
    """batch_paths = 1024: batches of 256 pixels x 4 samples (sn = 4 < S = 8), the last pixel chunk 128 pixels"""
    backend.upload_scene(scene)
    backend.set_option("batch_paths", 1024)
    try:
        a, _ = both(art, backend)
    finally:
        backend.set_option("batch_paths", DEFAULT_BATCH_PATHS)
    assert a["batches"] > 8
    try:
        big = render(art, backend, 1)                          # the picture does not depend on the batching
    finally:
        backend.set_option("camera_order", DEFAULT_ORDER)
    assert np.array_equal(big["accum"], a["accum"]) and big["rays"] == a["rays"]


def test_aa_off(art, backend, scene):
    """U = 1, sn = 2: not a multiple of 4"""
    backend.upload_scene(scene)
    a, _ = both(art, backend, aa=False)
    assert a["spp"] == 2


def test_sharded_frame(art, backend, scene):
    """rank 1 of 2 on a 96x64 frame: the rank's tile list is not contiguous, the local pixel -> pixel map not the identity"""
    backend.upload_scene(scene)
    try:
        backend.set_shard(1, 2, 32)
        a, _ = both(art, backend, width=96, height=64)
    finally:
        backend.set_shard(0, 1, 32)
    assert 0 < a["items_in"][0] < 8 * 96 * 64


def test_scene_without_a_bvh(art, backend):
    """the eight-sphere scene: no BVH, so the shade stage's staged copy-out is off"""
    from ada_ray_tracer_amd import scenes
    backend.upload_scene(scenes.eight_sphere_scene())
    both(art, backend)


def test_instanced_scene(art, backend):
    from ada_ray_tracer_amd import scenes
    backend.upload_scene(scenes.instanced_scene(2, 300))
    both(art, backend)


def test_counting_variant_counts_the_same(art, backend, scene):
    """count_tests = 1 counts per ray, not per order: the same box tests, triangle tests and node visits under both orders"""
    backend.upload_scene(scene)
    backend.set_option("count_tests", 1)
    try:
        a, b = both(art, backend)
    finally:
        backend.set_option("count_tests", 0)
    assert a["counters"] == b["counters"] and min(a["counters"]) > 0
