"""Rendering into a caller's torch tensor, on a caller's stream, in shards: the route of INTEGRATION.md section 5b and of bench.py under
torchrun (Backend.bind_accum / set_stream / set_shard, then render_pass_device and a sum over the ranks' tensors).

Every picture is compared as uint32 words, no tolerance.  The reference of a bound render is the same render through the library's own
buffer and its host copy (LAYOUT_ROW_MAJOR); one case is held to the CPU oracle as well, so the file does not rest on that path alone.
Who owns a pixel comes from tests/pixmap_ref.py (validated on the CPU by tests/test_pixmap.py), not from the product.

The backend is the session's: every test puts back the binding, the stream, the shard and the options it changed, and no tensor is
released while it is bound (Backend.bind_accum holds it; the tests keep their own reference as well)."""
import gc
import time
import weakref

import numpy as np
import pytest
import torch

import orc
import pixmap_ref
import test_gpu_shade_per as sp            # oracle_frame: the oracle's picture of a (scene, integrator, frame), computed once

pytestmark = pytest.mark.gpu

SEED = sp.SEED
DEPTH = 8
FRAMES = ((33, 16), (70, 45), (96, 64))
SCENES = ("reference", "synthetic", "instanced")
CASES = [(name, "PT_MIS") for name in SCENES] + [("reference", "PT_SHADOW"), ("reference", "PT_STUPID")]

_scenes = {}


def scene(art, name):
    if name not in _scenes:
        from ada_ray_tracer_amd import scenes
        _scenes[name] = {"reference": scenes.reference_scene, "synthetic": lambda: scenes.synthetic_scene(2000, 3),
                         "instanced": lambda: scenes.instanced_scene(n_instances=8, tris_per_mesh=2000)}[name]()
    return _scenes[name]


def params(art, rt, aa, vthreads, layout=None):
    return art.Backend.pass_params(getattr(art, rt), aa, DEPTH, vthreads, seed=SEED, layout=art.LAYOUT_ROW_MAJOR if layout is None else layout)


def restore(backend):
    """the state every other test of the session expects: nothing pending, the library's own buffer, the null stream, the whole frame"""
    torch.cuda.synchronize()
    backend.bind_accum(None)
    backend.set_stream(None)
    backend.set_shard(0, 1, 32)
    torch.cuda.synchronize()


def words(t, W, H):
    """the tensor's first 3 W H floats as [H, W, 3] uint32, after everything queued on the GPU"""
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()[:3 * W * H].view(np.uint32).reshape(H, W, 3).copy()


_internal = {}


def internal_frames(art, backend, name, rt, aa, vthreads, frame, passes=3):
    """The passes through the library's own buffer, whole frame, null stream: per pass the host accum's words [H, W, 3] (row-major), the
    LDR frame and stats().samples; and the batches the run took.  Rendered once per key, read-only."""
    key = (name, rt, aa, vthreads, frame, passes)
    if key not in _internal:
        W, H = frame
        restore(backend)
        backend.upload_scene(scene(art, name))
        backend.resize(W, H)
        p = params(art, rt, aa, vthreads)
        out, spp = [], 0
        for _ in range(passes):
            accum, screen, spp = backend.render_pass(p, spp, True, True)
            a = accum.view(np.uint32).copy(); a.setflags(write=False); screen.setflags(write=False)
            out.append((a, screen, spp, backend.stats().samples))
        assert backend.stats().lost_paths == 0 and out[-1][2] == passes * vthreads * (4 if aa else 1)
        assert any(a.any() for a, _, _, _ in out), "the reference picture is black"
        _internal[key] = (out, backend.stage_stats().batches)
    return _internal[key]


def differ(got, want):
    return "%d of %d words differ" % (int((got != want).sum()), want.size)


# ---- A. the bound tensor holds what the library's own buffer would ---------------------------------------------------------------------------
def check_bound_run(art, backend, name, rt, aa, vthreads, frame, want, batches=None):
    """Three passes into a bound zero tensor; after each the tensor is the internal path's accum of the same passes.  Then unbound: the
    tensor stays as it is and the library's own buffer gives the internal picture again."""
    W, H = frame
    lib = backend.lib
    t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    p = params(art, rt, aa, vthreads)
    try:
        backend.upload_scene(scene(art, name))
        backend.bind_accum(t)
        assert lib.art_accum_device() == t.data_ptr()
        assert not words(t, W, H).any(), "binding touched the tensor"
        backend.resize(W, H)
        spp = 0
        for k, (acc, _, wspp, wsamples) in enumerate(want):
            spp = backend.render_pass_device(p, spp)
            assert lib.art_accum_device() == t.data_ptr()
            got = words(t, W, H)
            assert spp == wspp and backend.stats().samples == wsamples
            assert np.array_equal(got, acc), "pass %d: the bound tensor is not the internal accum: %s" % (k + 1, differ(got, acc))
        assert backend.stats().lost_paths == 0
        if batches is not None:
            assert backend.stage_stats().batches == batches
        keep = t.clone()
        backend.bind_accum(None)
        assert lib.art_accum_device() != t.data_ptr() and lib.art_accum_device()
        backend.resize(W, H)
        accum, _, _ = backend.render_pass(p, 0)
        assert np.array_equal(accum.view(np.uint32), want[0][0]), "after the unbinding the library's own buffer is not used: " + differ(accum.view(np.uint32), want[0][0])
        torch.cuda.synchronize()
        assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), "the tensor was written after it was unbound"
    finally:
        restore(backend)
    return t


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("vthreads", [1, 2])
@pytest.mark.parametrize("aa", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("name,rt", CASES)
def test_bound_equals_internal(art, backend, name, rt, aa, vthreads, frame):
    want, batches = internal_frames(art, backend, name, rt, aa, vthreads, frame)
    assert batches == 3                                    # one batch per pass
    check_bound_run(art, backend, name, rt, aa, vthreads, frame, want, batches=3)


def test_bound_tensor_equals_the_oracle(art, backend):
    """The 2000-triangle scene at 33x16, 4 samples per pass: the bound tensor after pass 1 is the frame tests/test_gpu_shade_per.py holds
    its renders to (its oracle_frame), and after pass 3 the oracle's three passes."""
    W, H = 33, 16
    assert sp.FRAMES["33x16"] == (W, H, True)
    first = sp.oracle_frame(art, "synthetic", "PT_MIS", "33x16", DEPTH)[0]
    ref, rspp, _ = orc.render(sp.scene(art, "synthetic")[1].scene, orc.make_params(W, H, orc.PT_MIS, True, DEPTH, 1, seed=SEED), passes=3)
    t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    p = params(art, "PT_MIS", True, 1)
    try:
        backend.upload_scene(scene(art, "synthetic"))
        backend.bind_accum(t)
        backend.resize(W, H)
        spp = backend.render_pass_device(p, 0)
        got = words(t, W, H)
        assert np.array_equal(got, first.reshape(H, W, 3)), "pass 1: " + differ(got, first.reshape(H, W, 3))
        spp = backend.render_pass_device(p, backend.render_pass_device(p, spp))
        got = words(t, W, H)
        assert spp == rspp == 12
        assert np.array_equal(got, ref.view(np.uint32)), "pass 3: " + differ(got, ref.view(np.uint32))
    finally:
        restore(backend)


def test_several_batches_add_into_the_bound_tensor(art, backend):
    """batch_paths at its smallest (1024, as tests/test_gpu_camera_dedup.py::test_small_batches): 70x45 with 8 samples per pass is
    ceil(3150 / 256) = 13 pixel chunks of 256 pixels x 2 sample chunks of 4, so every pass launches the accumulate kernel 26 times on
    the bound tensor.  The picture is the one-batch internal picture."""
    frame = (70, 45)
    want, batches = internal_frames(art, backend, "synthetic", "PT_MIS", True, 2, frame)
    assert batches == 3
    backend.set_option("batch_paths", 1024)
    try:
        check_bound_run(art, backend, "synthetic", "PT_MIS", True, 2, frame, want, batches=3 * 13 * 2)
    finally:
        backend.set_option("batch_paths", sp.DEFAULT_BATCH_PATHS)


# ---- B. read-backs from a bound buffer ---------------------------------------------------------------------------------------------------------
def test_read_backs_from_a_bound_buffer(art, backend):
    """art_download and the host pointers of a pass read the bound tensor: row-major gives its words, ADA_XY its words transposed, and the
    LDR frames are the internal path's.  The debug pass writes its image into the tensor, row-major whatever the layout asked for."""
    frame = W, H = (70, 45)
    name, rt = "synthetic", "PT_MIS"
    want, _ = internal_frames(art, backend, name, rt, True, 1, frame)
    pd = {lay: art.Backend.pass_params(art.RT_DEBUG, False, DEPTH, 1, seed=SEED, layout=lay) for lay in (art.LAYOUT_ROW_MAJOR, art.LAYOUT_ADA_XY)}
    restore(backend)
    backend.upload_scene(scene(art, name))
    backend.resize(W, H)
    dbg = {lay: backend.debug_hit_pass(pd[lay]) for lay in pd}            # through the library's own buffer
    assert dbg[art.LAYOUT_ROW_MAJOR][0].any()
    t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    try:
        backend.bind_accum(t)
        backend.resize(W, H)
        p = params(art, rt, True, 1)
        spp = backend.render_pass_device(p, backend.render_pass_device(p, 0))
        tw = words(t, W, H)
        assert np.array_equal(tw, want[1][0])
        acc, screen = backend.download(spp, art.LAYOUT_ROW_MAJOR)
        assert np.array_equal(acc.view(np.uint32), tw) and np.array_equal(screen, want[1][1])
        acc, screen = backend.download(spp, art.LAYOUT_ADA_XY)
        assert acc.shape == (W, H, 3) and np.array_equal(acc.view(np.uint32), tw.transpose(1, 0, 2)) and np.array_equal(screen, want[1][1].T)
        # the host pointers of a pass, in the layout the pass asks for; the tensor stays row-major
        acc, screen, spp = backend.render_pass(params(art, rt, True, 1, layout=art.LAYOUT_ADA_XY), spp, True, True)
        tw = words(t, W, H)
        assert np.array_equal(tw, want[2][0]), differ(tw, want[2][0])
        assert np.array_equal(acc.view(np.uint32), tw.transpose(1, 0, 2)) and np.array_equal(screen, want[2][1].T)
        for lay in pd:
            t.fill_(123.0)                                               # a written image, not one added to what was there
            torch.cuda.synchronize()
            acc, screen, prim, mat, ptype = backend.debug_hit_pass(pd[lay])
            tw = words(t, W, H)
            row = acc if lay == art.LAYOUT_ROW_MAJOR else acc.transpose(1, 0, 2)
            assert np.array_equal(tw, np.ascontiguousarray(row).view(np.uint32)), "layout %d: the tensor is not the returned debug image, row-major" % lay
            assert np.array_equal(tw, dbg[art.LAYOUT_ROW_MAJOR][0].view(np.uint32)), "layout %d: %s" % (lay, differ(tw, dbg[art.LAYOUT_ROW_MAJOR][0].view(np.uint32)))
            for got, ref in zip((acc, screen, prim, mat, ptype), dbg[lay]):
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
    finally:
        restore(backend)


# ---- C. shards, one tensor per rank --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile,frame", [c for c in pixmap_ref.SHARD_CASES if c[2] in pixmap_ref.SHARD_FRAMES],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_shards_into_one_tensor_per_rank(art, backend, n, tile, frame):
    """Every rank of an n-way job renders two passes into its own zero tensor.  Outside the rank's pixels (tests/pixmap_ref.py) every word
    is 0x00000000, inside it is the unsharded frame's; the tensors sum to the unsharded frame in either rank order; the samples add up.
    A rank without a pixel (40x40 in tiles of 32 over 8 ranks: 2, 5, 6, 7) renders without error, leaves zeros and counts no sample."""
    W, H = frame
    want, _ = internal_frames(art, backend, "synthetic", "PT_MIS", True, 1, frame, passes=2)
    full, _, wspp, wsamples = want[-1]
    p = params(art, "PT_MIS", True, 1)
    parts, samples, empty = [], 0, []
    try:
        backend.upload_scene(scene(art, "synthetic"))
        for r in range(n):
            t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
            parts.append(t)
            backend.bind_accum(t)
            backend.set_shard(r, n, tile)
            backend.resize(W, H)
            spp = backend.render_pass_device(p, backend.render_pass_device(p, 0))
            st = backend.stats()
            assert spp == wspp and st.lost_paths == 0
            mask = pixmap_ref.owner_mask(W, H, r, n, tile)
            got = words(t, W, H)
            assert not got[~mask].any(), "rank %d: %d words outside its pixels are not 0x00000000" % (r, int(np.count_nonzero(got[~mask])))
            assert np.array_equal(got[mask], full[mask]), "rank %d: %s inside its pixels" % (r, differ(got[mask], full[mask]))
            assert st.samples == int(mask.sum()) * spp
            if not mask.any():
                empty.append(r)
                assert st.samples == 0 and st.rays == 0 and not got.any()
            samples += st.samples
        backend.bind_accum(None)
        torch.cuda.synchronize()
        if (n, tile, frame) == (8, 32, (40, 40)):
            assert empty == [2, 5, 6, 7]
        assert samples == wsamples
        fwd = torch.stack(parts).sum(0)
        rev = torch.stack(parts[::-1]).sum(0)
        assert np.array_equal(words(fwd, W, H), full), differ(words(fwd, W, H), full)
        assert np.array_equal(words(rev, W, H), full), differ(words(rev, W, H), full)
    finally:
        restore(backend)


# ---- D. the pass runs on the stream it was given -------------------------------------------------------------------------------------------------
# The filler: FILLER_LAUNCHES in-place multiplications of 2^24 floats on S, the kernel loaded beforehand.  Measured on an MI355X at 96x64,
# the tensor bound and S the library's stream: art_resize takes 0.03 - 0.14 ms of host time (0.027 - 0.033 ms in ten calls on an idle
# stream; 0.092 and 0.142 ms in two runs of this test, behind the filler); 200 such launches take 4.0 ms on the GPU and 0.78 ms to
# enqueue, i.e. 0.020 ms each against 0.004 ms, and the 400 here with the fill took 7.97 ms: about a hundred times the resize (56 to
# 290 times over those measurements).  The test prints both figures of its own run.
FILLER_FLOATS = 1 << 24
FILLER_LAUNCHES = 400


def _filler(x, launches):
    for _ in range(launches):
        x.mul_(1.0)


def test_the_pass_runs_on_the_stream_it_was_given(art, backend):
    """On a torch side stream S, bound and set_stream(S): a long chain of torch work, then tensor.fill_(7.0), all queued on S; then resize
    and two passes.  On S the resize's clear runs after the fill and the tensor ends as the internal picture; a library that ignored
    the stream would clear and render at once and the fill would land on top.  Precondition, asserted: the chain is still running when
    resize returns.  Then ray queries from the default stream, while S is the library's stream, give the bytes they give otherwise."""
    frame = W, H = (96, 64)
    name, rt = "synthetic", "PT_MIS"
    want, _ = internal_frames(art, backend, name, rt, True, 1, frame, passes=2)
    rng = np.random.default_rng(53)
    o = rng.uniform([-2.0, 0.5, 0.5], [2.0, 4.5, 6.0], (5000, 3)).astype(np.float32)
    d = rng.normal(size=(5000, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    restore(backend)
    backend.upload_scene(scene(art, name))
    og, dg = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    hits = backend.trace_rays_torch(og, dg).raw.clone()
    occ = backend.occluded_torch(og, dg).clone()
    torch.cuda.synchronize()
    assert 0 < int(occ.sum()) and np.array_equal(occ.cpu().numpy(), hits[:, 1].cpu().numpy() != 0)
    t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    x = torch.ones(FILLER_FLOATS, dtype=torch.float32, device="cuda")
    S = torch.cuda.Stream()
    p = params(art, rt, True, 1)
    try:
        backend.bind_accum(t)
        backend.set_stream(S.cuda_stream)
        backend.resize(W, H)                               # (the frame's buffers exist: the resize below allocates nothing new)
        backend.render_pass_device(p, 0)
        with torch.cuda.stream(S):
            _filler(x, 2)                                  # (the kernel's code is loaded: the chain below is 400 equal launches)
        torch.cuda.synchronize()
        start, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            start.record(S)
            _filler(x, FILLER_LAUNCHES)
            t.fill_(7.0)
            done.record(S)
        t0 = time.perf_counter()
        backend.resize(W, H)
        resize_ms = 1.0e3 * (time.perf_counter() - t0)
        still_running = not done.query()
        assert still_running, "precondition: the filler on S had finished when art_resize returned (%.3f ms of host time); the test would prove nothing" % resize_ms
        spp = backend.render_pass_device(p, backend.render_pass_device(p, 0))
        S.synchronize()
        print("art_resize: %.3f ms of host time; the filler and the fill: %.3f ms on the GPU" % (resize_ms, start.elapsed_time(done)))
        got = words(t, W, H)
        assert spp == want[1][2]
        assert np.array_equal(got, want[1][0]), "the pass did not run on the stream it was given: %s (%d words are 7.0)" % (
            differ(got, want[1][0]), int((got == np.float32(7.0).view(np.uint32)).sum()))
        # queries from the default stream while S is the library's stream
        h2 = backend.trace_rays_torch(og, dg).raw
        o2 = backend.occluded_torch(og, dg)
        torch.cuda.synchronize()
        assert torch.equal(h2, hits) and torch.equal(o2, occ)
        spp = backend.render_pass_device(p, spp)           # and a pass on S after them is the third pass
        backend.synchronize()
    finally:
        restore(backend)


# ---- E. refusals: nothing launched, the binding stays ----------------------------------------------------------------------------------------------
def test_refusals(art, backend):
    frame = W, H = (33, 16)
    name, rt = "synthetic", "PT_MIS"
    want, _ = internal_frames(art, backend, name, rt, True, 1, frame)
    lib = backend.lib
    p = params(art, rt, True, 1)
    t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    host = np.zeros(3 * W * H, np.float32)
    try:
        backend.upload_scene(scene(art, name))
        backend.bind_accum(t)
        backend.resize(W, H)
        # the C call: host memory
        assert lib.art_bind_accum(host.ctypes.data) != 0
        assert "not device memory" in lib.art_last_error().decode()
        assert lib.art_accum_device() == t.data_ptr()
        with pytest.raises(art.ArtError, match="not device memory"):
            backend.bind_accum(host.ctypes.data)
        assert lib.art_accum_device() == t.data_ptr() and backend._accum_tensor is t
        spp = backend.render_pass_device(p, 0)
        assert np.array_equal(words(t, W, H), want[0][0]) and not host.any()
        # the Python call: checked before any C call
        bad = {"a CPU tensor": torch.zeros(3 * W * H), "a float64 tensor": torch.zeros(3 * W * H, dtype=torch.float64, device="cuda"),
               "a non-contiguous view": torch.zeros(6 * W * H, dtype=torch.float32, device="cuda")[::2],
               "an empty tensor": torch.zeros(0, dtype=torch.float32, device="cuda"), "a numpy array": host, "a string": "accum"}
        for what, b in bad.items():
            with pytest.raises(art.ArtError, match="bind_accum"):
                backend.bind_accum(b)
            assert lib.art_accum_device() == t.data_ptr() and backend._accum_tensor is t, what
        # a frame the held tensor is too small for
        with pytest.raises(art.ArtError, match="bound accum tensor"):
            backend.resize(W + 1, H)
        assert (backend.width, backend.height) == (W, H)
        spp = backend.render_pass_device(p, spp)           # the frame, its spp and its contents are still there
        assert np.array_equal(words(t, W, H), want[1][0])
        acc, _ = backend.download(spp, art.LAYOUT_ROW_MAJOR)
        assert acc.shape == (H, W, 3) and np.array_equal(acc.view(np.uint32), want[1][0])
        # the tensor is held while bound and let go afterwards
        t2 = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
        backend.bind_accum(t2)
        w = weakref.ref(t2)
        del t2
        gc.collect()
        assert w() is not None and lib.art_accum_device() == w().data_ptr()
        backend.bind_accum(None)
        gc.collect()
        assert w() is None
    finally:
        restore(backend)
