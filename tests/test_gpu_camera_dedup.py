"""Option camera_dedup (default 1): a batch generates and traces each DISTINCT camera ray once -- a camera ray depends on
(pixel, sample & 3) alone -- and bounce 0 reads every sample's hit from its distinct ray.  Everything a caller can see must be what
camera_dedup = 0 (every sample's camera ray traced) gives: the accum bits, the LDR frame, ArtStats::rays (one camera query per sample,
the reference's Find_Closest_Hit calls), lost_paths == 0.  Only Backend.camera_rays_traced() tells the two apart.

Every case is a 48x32 frame (96x64 for the sharded one) of a ~2000-triangle scene at depth 3."""
import numpy as np
import pytest

import conv
import orc

pytestmark = pytest.mark.gpu

W, H, DEPTH = 48, 32, 3
DEFAULT_BATCH_PATHS = 128 << 20
COUNTERS = ("box_tests", "tri_tests", "node_visits", "leaf_visits", "traced_rays")


@pytest.fixture(scope="module")
def scene(art):
    from ada_ray_tracer_amd import scenes
    sd = scenes.synthetic_scene(2000, 3)
    return sd, conv.OracleScene(sd)


def traced_expected(npix, samples, aa, cap, dedup):
    """the batch plan of a pass (pixel chunk x sample chunk with at most `cap` paths, the sample chunk a multiple of 4 with AA on), and per
    batch of pn pixels x sn samples 4 * pn distinct camera rays with AA on (sn is a multiple of 4), pn with AA off; without dedup pn * sn"""
    per = 4 if aa else 1
    cap = max(cap, per)
    pc = min(npix, max(1, cap // per))
    sc = min(samples, max(per, (cap // pc) // per * per))
    total = 0
    for px0 in range(0, npix, pc):
        pn = min(pc, npix - px0)
        for s0 in range(0, samples, sc):
            sn = min(sc, samples - s0)
            total += ((4 if aa else 1) * pn) if dedup else pn * sn
    return total


def render(art, be, dedup, rt, aa, passes, width=W, height=H, seed=5, cap=DEFAULT_BATCH_PATHS, expect_dedup=None):
    """`passes`: vthreads of each Render_Pass in turn (the spp carries over: the second pass starts at sample_base = the first one's spp).
    Returns what a caller sees; checks the traced-camera-ray count against the batch plan on the way."""
    be.set_option("camera_dedup", dedup)
    be.resize(width, height)
    spp, accum, screen, traced = 0, None, None, 0
    for vthreads in passes:
        accum, screen, spp1 = be.render_pass(art.Backend.pass_params(rt, aa, DEPTH, vthreads, seed=seed), spp, want_screen=True)
        npix = be.stats().samples // spp1                 # this device's pixels (a shard renders its own tiles only)
        traced += traced_expected(npix, spp1 - spp, aa, cap, dedup if expect_dedup is None else expect_dedup)
        spp = spp1
    st = be.stats()
    assert st.lost_paths == 0
    assert be.camera_rays_traced() == traced
    return dict(accum=np.ascontiguousarray(accum).view(np.uint32), screen=screen, rays=st.rays, spp=spp,
                traced=traced, counters=tuple(getattr(st, k) for k in COUNTERS))


def assert_same(a, b):
    assert a["spp"] == b["spp"] and a["rays"] == b["rays"]
    assert np.array_equal(a["accum"], b["accum"]) and np.array_equal(a["screen"], b["screen"])


def both(art, be, *args, **kw):
    try:
        off = render(art, be, 0, *args, **kw)
        on = render(art, be, 1, *args, **kw)
    finally:
        be.set_option("camera_dedup", 1)
    assert_same(on, off)
    return on, off


def test_aa_on_8spp_one_pass_equals_the_oracle(art, backend, scene):
    """U = 4 distinct rays per pixel for 8 samples: half the camera rays are traced"""
    sd, osc = scene
    backend.upload_scene(sd)
    on, off = both(art, backend, art.PT_MIS, True, [2])
    assert on["traced"] == 4 * W * H and off["traced"] == 8 * W * H
    ref, rspp, cnt = orc.render(osc.scene, orc.make_params(W, H, orc.PT_MIS, True, DEPTH, 2, seed=5))
    assert on["spp"] == rspp == 8
    assert np.array_equal(on["accum"], np.ascontiguousarray(ref, np.float32).view(np.uint32))
    assert np.array_equal(on["screen"], orc.resolve(ref, rspp))
    assert on["rays"] == off["rays"] == cnt.rays


def test_aa_on_two_passes_of_4spp(art, backend, scene):
    """the second pass starts at sample_base = 4: its local samples 0..3 are again sample & 3 = 0..3"""
    backend.upload_scene(scene[0])
    on, off = both(art, backend, art.PT_MIS, True, [1, 1])
    assert on["spp"] == 8 and on["traced"] == off["traced"] == 8 * W * H      # 4 samples per batch: nothing to share


def test_aa_off_8spp(art, backend, scene):
    """U = 1: one camera ray per pixel serves all 8 samples"""
    backend.upload_scene(scene[0])
    on, off = both(art, backend, art.PT_MIS, False, [8])
    assert on["traced"] == W * H and off["traced"] == 8 * W * H


@pytest.mark.parametrize("aa", [True, False])
def test_small_batches(art, backend, scene, aa):
    """batch_paths = 1024 < 48 * 32 pixels: several pixel chunks (px0 > 0) and the smallest sample chunk there is.  With AA off that is
    sn = 1 < 4 (U = 1); with AA on a sample chunk is never below the 4 samples of a pixel's Generate4RayDirections group, so
    sn = 4 = U and the pixel chunk is 256."""
    backend.upload_scene(scene[0])
    backend.set_option("batch_paths", 1024)
    try:
        on, off = both(art, backend, art.PT_MIS, aa, [2] if aa else [8], cap=1024)
    finally:
        backend.set_option("batch_paths", DEFAULT_BATCH_PATHS)
    assert on["traced"] == 8 * W * H                      # one sample group per batch: every ray of a batch is distinct
    big = render(art, backend, 1, art.PT_MIS, aa, [2] if aa else [8])      # the picture does not depend on the batching
    assert_same(big, on)


def test_sharded_frame(art, backend, scene):
    """rank 1 of 2 on a 96x64 frame: the local pixel -> pixel map is not the identity"""
    backend.upload_scene(scene[0])
    try:
        backend.set_shard(1, 2, 32)
        on, off = both(art, backend, art.PT_MIS, True, [2], width=96, height=64)
    finally:
        backend.set_shard(0, 1, 32)
    assert 0 < on["traced"] == off["traced"] // 2 < 4 * 96 * 64


def test_instanced_scene(art, backend):
    from ada_ray_tracer_amd import scenes
    backend.upload_scene(scenes.instanced_scene(2, 300))
    on, off = both(art, backend, art.PT_MIS, True, [2])
    assert on["traced"] == 4 * W * H


@pytest.mark.parametrize("rt", ["PT_STUPID", "PT_SHADOW"])
def test_other_integrators(art, backend, scene, rt):
    backend.upload_scene(scene[0])
    on, off = both(art, backend, getattr(art, rt), True, [2])
    assert on["traced"] == 4 * W * H


def test_counting_pass_traces_every_camera_ray(art, backend, scene):
    """count_tests = 1: the counting variant's contract is the oracle's walk of every ray, so the option does not apply"""
    backend.upload_scene(scene[0])
    backend.set_option("count_tests", 1)
    try:
        on, off = both(art, backend, art.PT_MIS, True, [2], expect_dedup=0)
    finally:
        backend.set_option("count_tests", 0)
    assert on["counters"] == off["counters"] and min(on["counters"]) > 0
    assert on["traced"] == off["traced"] == 8 * W * H
