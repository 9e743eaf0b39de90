"""Luminance moments of the render passes (art_bind_moments / Backend.bind_moments) on the GPU.

After every pass the bound moments tensor is held, word for word, to tests/moments_ref.py: the CPU oracle's per-sample radiance, cut into
colours and summed in numpy binary32 in the order include/art_hip.h states.  The bound accum of the same run is held, word for word, to the
same render without moments (tests/test_gpu_bound_accum.internal_frames), so binding moments changes nothing else.  Who owns a pixel of a
shard comes from tests/pixmap_ref.py.

The backend is the session's: every test ends in restore(), which also unbinds the moments."""
import time

import numpy as np
import pytest
import torch

import conv
import hostsim
import moments_ref as M
import orc
import pixmap_ref
import test_gpu_bound_accum as ba
import test_gpu_shade_per as sp

pytestmark = pytest.mark.gpu

F = np.float32
SEED, DEPTH = ba.SEED, ba.DEPTH
FRAMES = ((33, 16), (70, 45))
CASES = [(name, "PT_MIS") for name in ba.SCENES] + [("reference", "PT_STUPID")]
PASSES = 3
MAX_VTHREADS = 3


def restore(backend):
    torch.cuda.synchronize()
    backend.bind_moments(None)
    ba.restore(backend)


_oracle_scenes = {}


def oracle_scene(art, name):
    """what the oracle renders for the scene ba.scene(art, name) uploads: the reference's own scene, or the mesh scene (an instanced one
    flattened to its explicit world-space mesh) with the host builder's tree attached, so that a sample costs microseconds"""
    if name not in _oracle_scenes:
        if name == "reference":
            _oracle_scenes[name] = orc.CornellScene()
        else:
            sd = ba.scene(art, name)
            flat = hostsim.flattened_copy(art, sd) if name == "instanced" else sd
            osc = conv.OracleScene(flat)
            nodes, tris, info = hostsim.bvh(art, flat)
            osc.attach_bvh(nodes, tris, info["width"])
            _oracle_scenes[name] = osc
    return _oracle_scenes[name]


_rad = {}


def radiance(art, name, rt, aa, frame):
    """the oracle's radiance of every camera sample three passes of MAX_VTHREADS virtual threads take, [S, H, W, 3]; a run with fewer
    virtual threads uses a prefix.  Computed once per key, read-only."""
    key = (name, rt, aa, frame)
    if key not in _rad:
        W, H = frame
        prm = orc.make_params(W, H, getattr(orc, rt), aa, DEPTH, 1, seed=SEED)
        r = M.sample_radiance(oracle_scene(art, name).scene, prm, 0, PASSES * MAX_VTHREADS * (4 if aa else 1))
        r.setflags(write=False)
        _rad[key] = r
    return _rad[key]


def want_moments(art, name, rt, aa, vthreads, frame, passes=PASSES):
    """per pass: (the moments' words [H, W, 2], the reference's accum words [H, W, 3])"""
    per = vthreads * (4 if aa else 1)
    rad = radiance(art, name, rt, aa, frame)
    acc = mom = None
    out = []
    for k in range(passes):
        acc, mom = M.add_colours(M.colours(rad[k * per:(k + 1) * per], aa), acc, mom)
        out.append((mom.view(np.uint32).copy(), acc.view(np.uint32).copy()))
    return out


def mwords(t, W, H):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()[:2 * W * H].view(np.uint32).reshape(H, W, 2).copy()


def differ(got, want):
    return "%d of %d words differ" % (int((got != want).sum()), want.size)


def check_run(art, backend, name, rt, aa, vthreads, frame, batches=None):
    """three passes with an accum tensor and a moments tensor bound: after each pass the moments are the reference's and the accum is
    the render's without moments (and the reference's)"""
    W, H = frame
    internal, _ = ba.internal_frames(art, backend, name, rt, aa, vthreads, frame)
    want = want_moments(art, name, rt, aa, vthreads, frame)
    t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    m = torch.full((2 * W * H,), 5.0, dtype=torch.float32, device="cuda")
    p = ba.params(art, rt, aa, vthreads)
    try:
        backend.upload_scene(ba.scene(art, name))
        backend.bind_accum(t)
        backend.bind_moments(m)
        torch.cuda.synchronize()
        assert (m == 5.0).all(), "binding touched the tensor"
        backend.resize(W, H)
        assert not mwords(m, W, H).any(), "resize did not zero the moments"
        spp = 0
        for k in range(PASSES):
            spp = backend.render_pass_device(p, spp)
            got, acc = mwords(m, W, H), ba.words(t, W, H)
            assert spp == internal[k][2]
            assert np.array_equal(acc, internal[k][0]), "pass %d: the accum differs from the render without moments: %s" % (k + 1, differ(acc, internal[k][0]))
            assert np.array_equal(acc, want[k][1]), "pass %d: the accum is not the reference's: %s" % (k + 1, differ(acc, want[k][1]))
            assert np.array_equal(got, want[k][0]), "pass %d: moments: %s" % (k + 1, differ(got, want[k][0]))
        assert backend.stats().lost_paths == 0 and got.any()
        if batches is not None:
            assert backend.stage_stats().batches == batches
    finally:
        restore(backend)


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("vthreads", [1, 3])
@pytest.mark.parametrize("aa", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("name,rt", CASES)
def test_moments_equal_the_reference(art, backend, name, rt, aa, vthreads, frame):
    check_run(art, backend, name, rt, aa, vthreads, frame, batches=PASSES)


def test_a_pixels_samples_in_several_chunks(art, backend):
    """batch_paths 1024 at 70x45 with 12 samples per pass: 13 pixel chunks of 256 pixels x 3 sample chunks of 4, so a pixel's colours of
    one pass arrive in three launches; the sums run on in batch order and the words are those of the one-batch reference"""
    backend.set_option("batch_paths", 1024)
    try:
        check_run(art, backend, "synthetic", "PT_MIS", True, 3, (70, 45), batches=PASSES * 13 * 3)
        check_run(art, backend, "synthetic", "PT_MIS", False, 3, (70, 45))
    finally:
        backend.set_option("batch_paths", sp.DEFAULT_BATCH_PATHS)


def test_plain_schedule(art, backend):
    """option trace_kernel 1: the one-ray-per-lane schedule has a call site of its own"""
    backend.set_option("trace_kernel", 1)
    try:
        check_run(art, backend, "synthetic", "PT_MIS", True, 1, (33, 16))
    finally:
        backend.set_option("trace_kernel", 0)


def test_shards(art, backend):
    """set_shard(r, 3, 32) at 70x45: a rank's moments are the whole frame's inside its pixels and +0 outside; the three buffers sum to
    the whole frame (every pixel has one owner, so the sum adds zeros)"""
    frame = W, H = (70, 45)
    name, rt = "synthetic", "PT_MIS"
    want = want_moments(art, name, rt, True, 1, frame)[1][0]
    p = ba.params(art, rt, True, 1)
    parts = []
    try:
        backend.upload_scene(ba.scene(art, name))
        for r in range(3):
            t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
            m = torch.zeros(2 * W * H, dtype=torch.float32, device="cuda")
            parts.append((t, m))
            backend.bind_accum(t)
            backend.bind_moments(m)
            backend.set_shard(r, 3, 32)
            backend.resize(W, H)
            backend.render_pass_device(p, backend.render_pass_device(p, 0))
            mask = pixmap_ref.owner_mask(W, H, r, 3, 32)
            got = mwords(m, W, H)
            assert mask.any() and not got[~mask].any(), "rank %d: words outside its pixels are not 0x00000000" % r
            assert np.array_equal(got[mask], want[mask]), "rank %d: %s" % (r, differ(got[mask], want[mask]))
        backend.bind_moments(None)
        total = torch.stack([m for _, m in parts]).sum(0)
        assert np.array_equal(mwords(total, W, H), want)
    finally:
        restore(backend)


def test_side_stream(art, backend):
    """On a torch side stream S that is the library's stream: a long chain of torch work and then moments.fill_(7.0) are queued on S, then
    resize and two passes.  On S the resize's clear comes after the fill and the moments end as the reference's; a clear or an
    accumulate on another stream would meet the fill.  Precondition, asserted: the chain is still running when resize returns."""
    frame = W, H = (33, 16)
    name, rt = "synthetic", "PT_MIS"
    want = want_moments(art, name, rt, True, 1, frame)[1][0]
    m = torch.zeros(2 * W * H, dtype=torch.float32, device="cuda")
    x = torch.ones(ba.FILLER_FLOATS, dtype=torch.float32, device="cuda")
    S = torch.cuda.Stream()
    p = ba.params(art, rt, True, 1)
    try:
        backend.upload_scene(ba.scene(art, name))
        backend.bind_moments(m)
        backend.set_stream(S.cuda_stream)
        backend.resize(W, H)
        backend.render_pass_device(p, 0)
        with torch.cuda.stream(S):
            ba._filler(x, 2)
        torch.cuda.synchronize()
        done = torch.cuda.Event()
        with torch.cuda.stream(S):
            ba._filler(x, ba.FILLER_LAUNCHES)
            m.fill_(7.0)
            done.record(S)
        t0 = time.perf_counter()
        backend.resize(W, H)
        resize_ms = 1.0e3 * (time.perf_counter() - t0)
        assert not done.query(), "precondition: the filler on S had finished when art_resize returned (%.3f ms of host time)" % resize_ms
        backend.render_pass_device(p, backend.render_pass_device(p, 0))
        S.synchronize()
        got = mwords(m, W, H)
        assert np.array_equal(got, want), "%s (%d words are 7.0)" % (differ(got, want), int((got == F(7.0).view(np.uint32)).sum()))
        backend.synchronize()
    finally:
        restore(backend)


def test_unbound_untouched_refusals_and_the_debug_pass(art, backend):
    frame = W, H = (33, 16)
    name, rt = "synthetic", "PT_MIS"
    want = want_moments(art, name, rt, True, 1, frame)
    lib = backend.lib
    p = ba.params(art, rt, True, 1)
    m = torch.zeros(2 * W * H, dtype=torch.float32, device="cuda")
    host = np.zeros(2 * W * H, F)
    try:
        backend.upload_scene(ba.scene(art, name))
        backend.bind_moments(m)
        backend.resize(W, H)
        # host memory: refused, the binding stays and the next pass still writes the tensor
        assert lib.art_bind_moments(host.ctypes.data) != 0
        assert "not device memory" in lib.art_last_error().decode()
        with pytest.raises(art.ArtError, match="not device memory"):
            backend.bind_moments(host.ctypes.data)
        assert backend._moments_tensor is m
        spp = backend.render_pass_device(p, 0)
        assert np.array_equal(mwords(m, W, H), want[0][0]) and not host.any()
        # the Python checks, before any C call
        bad = {"a CPU tensor": torch.zeros(2 * W * H), "a float64 tensor": torch.zeros(2 * W * H, dtype=torch.float64, device="cuda"),
               "a non-contiguous view": torch.zeros(4 * W * H, dtype=torch.float32, device="cuda")[::2],
               "an empty tensor": torch.zeros(0, dtype=torch.float32, device="cuda"), "a numpy array": host, "a string": "moments"}
        for what, b in bad.items():
            with pytest.raises(art.ArtError, match="bind_moments"):
                backend.bind_moments(b)
            assert backend._moments_tensor is m, what
        with pytest.raises(art.ArtError, match="bound moments tensor"):
            backend.resize(W + 1, H)
        # the debug pass leaves the moments as they were
        backend.debug_hit_pass(art.Backend.pass_params(art.RT_DEBUG, False, DEPTH, 1, seed=SEED))
        assert np.array_equal(mwords(m, W, H), want[0][0])
        spp = backend.render_pass_device(p, spp)
        assert np.array_equal(mwords(m, W, H), want[1][0])
        # a resize zeroes them
        backend.resize(W, H)
        assert not mwords(m, W, H).any()
        backend.render_pass_device(p, 0)
        assert np.array_equal(mwords(m, W, H), want[0][0])
        # unbound: a render leaves the tensor untouched
        keep = m.clone()
        backend.bind_moments(None)
        assert backend._moments_tensor is None
        backend.resize(W, H)
        backend.render_pass_device(p, 0)
        torch.cuda.synchronize()
        assert torch.equal(m.view(torch.int32), keep.view(torch.int32)), "the tensor was written after it was unbound"
    finally:
        restore(backend)
