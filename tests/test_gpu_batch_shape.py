"""The batch shape of a pass: samples first.  A batch is a pixel chunk x a sample chunk of at most `batch_paths` paths; when a pixel's S
samples fit for at least 256 pixels (or the whole frame), the chunk carries all of them (pc = batch_paths / S pixels, a multiple of 1024
once it is that large), so each distinct camera ray of the pass is traced once: U * npix per pass.  Only with batch_paths < 256 * S do
sample chunks reappear (pixels first, as before), and a pixel chunk's camera rays are traced once per sample chunk.  Nothing a caller sees may depend on the shape: accum bits, the LDR
frame, ArtStats::rays and samples.

96x64 frames (32x16 for the fallback, whose pass has 1040 samples) of a ~2000-triangle scene, PT_MIS, depth 4, AA on."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, DEPTH, SEED = 96, 64, 4, 11
DEFAULT_BATCH_PATHS = 128 << 20
# one batch | 625-pixel chunks, the last one partial | 2048-pixel chunks (2500 aligned down to whole tiles)
CAPS = (DEFAULT_BATCH_PATHS, 5000, 20000)


def plan(npix, S, cap, per=4):
    """(pixel chunk, sample chunk) of a pass, the mirror of plan_batch in csrc/art_pass_plan.h (tests/test_pass_plan_host.py holds the two
    together): the issue's samples-first rule, taken only when all S samples of at least 256 pixels
    (or of the frame) fit -- the minimum that keeps test_gpu_camera_dedup.py's pinned plan at batch_paths = 1024; else pixels first"""
    cap = max(cap, per)
    if cap // S >= min(npix, 256):
        pc = min(npix, max(1, cap // S))
        if pc < npix and pc >= 1024:
            pc = pc // 1024 * 1024
        return pc, S
    pc = min(npix, max(1, cap // per))
    return pc, min(S, max(per, (cap // pc) // per * per))


def batches(npix, S, cap):
    pc, sc = plan(npix, S, cap)
    return -(-npix // pc) * -(-S // sc)


def render(art, be, cap, passes, width=W, height=H, dedup=1, kernel=0):
    be.set_option("batch_paths", cap)
    be.set_option("camera_dedup", dedup)
    be.set_option("trace_kernel", kernel)
    try:
        be.resize(width, height)
        spp, accum, screen = 0, None, None
        for vthreads in passes:
            accum, screen, spp = be.render_pass(art.Backend.pass_params(art.PT_MIS, True, DEPTH, vthreads, seed=SEED), spp, want_screen=True)
        st = be.stats()
        assert st.lost_paths == 0
        return dict(accum=np.ascontiguousarray(accum).view(np.uint32).copy(), screen=np.array(screen, copy=True), rays=st.rays,
                    samples=st.samples, spp=spp, traced=be.camera_rays_traced(), batches=be.stage_stats().batches)
    finally:
        be.set_option("batch_paths", DEFAULT_BATCH_PATHS)
        be.set_option("camera_dedup", 1)
        be.set_option("trace_kernel", 0)


def assert_same(a, b, counters=True):
    assert a["spp"] == b["spp"]
    if counters:
        assert a["rays"] == b["rays"] and a["samples"] == b["samples"]
    assert np.array_equal(a["accum"], b["accum"]) and np.array_equal(a["screen"], b["screen"])


@pytest.fixture(scope="module")
def scene(art):
    from ada_ray_tracer_amd import scenes
    return scenes.synthetic_scene(2000, 3)


@pytest.fixture(scope="module")
def whole(art, backend, scene):
    """the pass as one batch, 8 samples: the frame every other shape must give (computed once, never changed)"""
    backend.upload_scene(scene)
    return render(art, backend, DEFAULT_BATCH_PATHS, [2])


def test_the_plan_has_the_shapes_this_file_is_about():
    assert plan(W * H, 8, CAPS[0]) == (W * H, 8)
    assert plan(W * H, 8, CAPS[1]) == (625, 8) and (W * H) % 625 != 0
    assert plan(W * H, 8, CAPS[2]) == (2048, 8)
    assert plan(32 * 16, 1040, 1024) == (256, 4)
    assert plan(W * H, 8, 1024) == (256, 4)               # room for 128 pixels x 8 samples only: pixels first


@pytest.mark.parametrize("cap", CAPS)
def test_pixel_chunks_of_the_full_pass(art, backend, scene, whole, cap):
    backend.upload_scene(scene)
    got = render(art, backend, cap, [2])
    assert_same(got, whole)
    assert got["traced"] == 4 * W * H                     # U * npix, however many pixel chunks
    assert got["batches"] == batches(W * H, 8, cap) == {CAPS[0]: 1, 5000: 10, 20000: 3}[cap]      # the product's pc: 6144, 625, 2048 (not 2500)
    off = render(art, backend, cap, [2], dedup=0)
    assert_same(off, whole)
    assert off["traced"] == 8 * W * H


def test_fewer_path_slots_than_samples_of_a_pixel(art, backend, scene):
    """batch_paths = 1024 < S = 1040: 256 pixels x 4 samples per batch, 260 sample chunks per pixel chunk"""
    backend.upload_scene(scene)
    w, h, vt = 32, 16, 260
    one = render(art, backend, DEFAULT_BATCH_PATHS, [vt], w, h)
    assert one["traced"] == 4 * w * h
    got = render(art, backend, 1024, [vt], w, h)
    assert_same(got, one)
    assert got["traced"] == 4 * w * h * 260               # U * npix * ceil(S / sc)
    assert one["batches"] == 1 and got["batches"] == 2 * 260
    simple = render(art, backend, 1024, [vt], w, h, kernel=1)
    assert_same(simple, one, counters=False)
    off = render(art, backend, 1024, [vt], w, h, dedup=0)
    assert_same(off, one)
    assert off["traced"] == w * h * 4 * vt


def test_less_room_than_256_pixels_with_all_their_samples(art, backend, scene, whole):
    """batch_paths = 1024, S = 8: 256 pixels x 4 samples per batch, two sample chunks per pixel chunk"""
    backend.upload_scene(scene)
    got = render(art, backend, 1024, [2])
    assert_same(got, whole)
    assert got["traced"] == 4 * W * H * 2 and got["batches"] == 24 * 2


def test_two_passes_of_8_vthreads_equal_one_of_16(art, backend, scene):
    """cap 20000: 312-pixel chunks at 64 samples, 625-pixel chunks at 32 -- twenty and ten pixel chunks"""
    backend.upload_scene(scene)
    assert plan(W * H, 64, 20000) == (312, 64) and plan(W * H, 32, 20000) == (625, 32)
    two = render(art, backend, 20000, [8, 8])
    one = render(art, backend, 20000, [16])
    assert_same(two, one)
    assert two["traced"] == 2 * 4 * W * H and one["traced"] == 4 * W * H
    assert two["batches"] == 2 * 10 and one["batches"] == 20


def test_sharded_frame(art, backend, scene, whole):
    """rank 1 of 3, 32-pixel tiles, 500-pixel chunks: the same frame as the rank renders in one batch (zeros outside its tiles included),
    and where it rendered, the unsharded frame's values"""
    backend.upload_scene(scene)
    try:
        backend.set_shard(1, 3, 32)
        one = render(art, backend, DEFAULT_BATCH_PATHS, [2])
        got = render(art, backend, 4000, [2])
    finally:
        backend.set_shard(0, 1, 32)
    npix = got["samples"] // 8
    assert 0 < npix < W * H and plan(npix, 8, 4000)[0] == 500
    assert got["traced"] == one["traced"] == 4 * npix
    assert got["batches"] == -(-npix // 500) and one["batches"] == 1
    assert_same(got, one)
    # the deal of a 3-rank job: tile (bx, by) belongs to rank (bx + 5 by) mod 3
    y, x = np.divmod(np.arange(W * H), W)
    mine = ((x // 32 + 5 * (y // 32)) % 3 == 1)
    assert int(mine.sum()) == npix
    a, ref = got["accum"].reshape(W * H, 3), whole["accum"].reshape(W * H, 3)      # row-major pixels x rgb
    assert np.array_equal(a[mine], ref[mine]) and not a[~mine].any()
    assert np.array_equal(got["screen"].reshape(-1)[mine], whole["screen"].reshape(-1)[mine])


@pytest.mark.parametrize("cap", CAPS + (1024,))          # 1024: sample chunks (256 pixels x 4 samples); S = 1040 > batch_paths is rendered above
def test_the_simple_schedule_gives_the_same_frame(art, backend, scene, whole, cap):
    backend.upload_scene(scene)
    got = render(art, backend, cap, [2], kernel=1)
    assert_same(got, whole, counters=False)               # (the plain schedule answers the shadow queries of every slot: its `rays` is its own)
    assert got["samples"] == whole["samples"]
