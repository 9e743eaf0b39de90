"""art_firefly_device on the GPU against the numpy reference written from the header (tests/firefly_ref.py): bit equality on the shapes and
parameter sets the host test shares, planted bad values included; in place against out of place; a side stream; the scratch growing in a
process of its own; the flags through compact_mask_torch; every refusal of tests/golden/firefly_refusals.json; the chain pass -> firefly
-> temporal end to end; and the planted spikes and the asserted quality figure on the GPU's own frames."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import firefly_quality as FQ
import firefly_ref as R
import firefly_refusals as RF
import temporal_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_firefly(backend, color, moments=None, ids=None, in_place=False, **kw):
    """firefly_ref.firefly's signature through Backend.firefly_torch; the reference's defaults, not the package's"""
    kw = dict(dict(radius=1, rank=1, min_count=None, scale=1.0, gain=2.0, floor=0.0), **kw)
    c, m, i = dev(np.asarray(color, F)), dev(None if moments is None else np.asarray(moments, F)), dev(ids)
    H, W = c.shape[:2]
    out = c if in_place else torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
    mo = None if m is None else (m if in_place else torch.full((H, W, 2), -7.0, dtype=torch.float32, device="cuda"))
    got = backend.firefly_torch(c, m, i, out=out, moments_out=mo, **kw)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is mo
    if not in_place:                                                  # (the input planes are only read)
        assert R.differ(c.cpu().numpy(), np.asarray(color, F)) == 0 and (m is None or R.differ(m.cpu().numpy().reshape(-1), np.asarray(moments, F).reshape(-1)) == 0)
    return got[0].cpu().numpy(), None if mo is None else got[1].cpu().numpy().reshape(H, W, 2), got[2].cpu().numpy()


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_kernels_equal_the_reference(backend, size):
    W, H = size
    for name, kw in R.cases(W, H):
        ref = R.firefly(**kw)
        assert R.differ_all(gpu_firefly(backend, **kw), ref) == 0, name
        assert R.differ_all(gpu_firefly(backend, in_place=True, **kw), ref) == 0, name + " (in place)"


def test_in_place_equals_out_of_place(backend):
    """83 x 41 is 6 x 3 tiles, the last column and row partial; every tile's halo reaches into tiles another workgroup overwrites in place"""
    color, moments, ids = R.frame(83, 41, seed=3)
    color, moments = R.planted_bad(color, moments)
    for kw in (dict(radius=2, rank=2, gain=1.0, scale=0.25), dict(radius=1, rank=1, gain=2.0, scale=0.25, ids=ids)):
        a = gpu_firefly(backend, color, moments, **kw)
        b = gpu_firefly(backend, color, moments, in_place=True, **kw)
        assert R.differ_all(a, b) == 0 and R.differ_all(a, R.firefly(color, moments, **kw)) == 0 and (a[2] == 1).sum() > 20


def test_side_stream_gives_the_context_streams_bits(backend):
    """inputs copied on a torch side stream and the call enqueued there with no synchronisation in between, writing over its own inputs"""
    W, H = 70, 21
    color, moments, ids = R.frame(W, H, seed=4)
    kw = dict(radius=2, rank=2, gain=2.0, floor=0.01, scale=0.25)
    ref = R.firefly(color, moments, ids, **kw)
    assert R.differ_all(gpu_firefly(backend, color, moments, ids, **kw), ref) == 0
    ch, mh, ih = torch.from_numpy(color).pin_memory(), torch.from_numpy(moments).pin_memory(), torch.from_numpy(ids).pin_memory()
    cd, md = torch.zeros((H, W, 3), device="cuda"), torch.zeros((H, W, 2), device="cuda")
    idd = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        cd.copy_(ch, non_blocking=True); md.copy_(mh, non_blocking=True); idd.copy_(ih, non_blocking=True)
        got = backend.firefly_torch(cd, md, idd, out=cd, moments_out=md, **kw)
    st.synchronize()
    assert got[0] is cd and R.differ_all((cd.cpu().numpy(), md.cpu().numpy(), got[2].cpu().numpy()), ref) == 0 and torch.equal(idd.cpu(), ih)


def test_scratch_grows_in_a_process_of_its_own(art):
    """art_init only, no scene and no viewport: a 1 x 1 call sizes the scratch at 4 bytes, the 70 x 66 call makes it grow, and the bits
    are the reference's after growing"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, torch, __graft_entry__ as g, firefly_ref as R\n"
            "art = g.load_package(); be = art.Backend(0)\n"
            "one = np.full((1, 1, 3), 2.0, np.float32)\n"
            "a = be.firefly_torch(torch.from_numpy(one).cuda(), rank=1, radius=1)\n"
            "color, moments, ids = R.frame(70, 66)\n"
            "kw = dict(radius=2, rank=2, gain=1.0, floor=0.0, scale=0.25)\n"
            "b = be.firefly_torch(*[torch.from_numpy(x).cuda() for x in (color, moments, ids)], **kw)\n"
            "torch.cuda.synchronize()\n"
            "print('ONE', a[0].cpu().numpy().tolist(), int(a[2].cpu()[0, 0]))\n"
            "print('DIFFER', R.differ_all([x.cpu().numpy() for x in b], R.firefly(color, moments, ids, **kw)))\n"
            "be.shutdown()\n") % (art.ROOT, os.path.join(art.ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DIFFER 0" in r.stdout and "ONE [[[2.0, 2.0, 2.0]]] 0" in r.stdout, (r.stdout, r.stderr[-2000:])


def test_flags_through_compact_mask(backend):
    """clamped1b as a mask: compact_mask_torch selects exactly the reference's flagged pixels (flags 1 and 2), in the list's order"""
    W, H = 70, 66
    color, moments, ids = R.frame(W, H, seed=6)
    color, moments = R.planted_bad(color, moments)
    kw = dict(radius=1, rank=1, gain=2.0, floor=0.0, scale=0.25)
    ref = R.firefly(color, moments, None, **kw)
    backend.resize(W, H)
    out, mo, flags = backend.firefly_torch(dev(color), dev(moments), None, **kw)
    pixels, count = backend.compact_mask_torch(flags)
    torch.cuda.synchronize()
    n = int(count.cpu()[0])
    want = np.flatnonzero(ref[2].reshape(-1))
    assert (ref[2] == 1).any() and (ref[2] == 2).any() and n == want.size
    assert sorted(pixels.cpu().numpy()[:n].astype(np.int64).tolist()) == want.tolist()


def test_every_refusal_of_the_fixture(art, backend):
    """every case of tests/golden/firefly_refusals.json over device planes: refused with its message and every output still holds its
    sentinel; then the good call and the in-place call are accepted"""
    frame, cases = RF.load()
    sizes = RF.plane_bytes(frame)
    offsets, at = {}, 0
    for k in RF.PLANES:
        offsets[k] = at
        at += (sizes[k] + 255) // 256 * 256
    arena = torch.full((at + 4 * sizes["color3f"],), 0x5a, dtype=torch.uint8, device="cuda")
    base = {k: arena.data_ptr() + offsets[k] for k in RF.PLANES}
    host = np.zeros(sizes["color3f"] // 4, F)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    held = []

    def short(nbytes):
        p = C.c_void_p(None)
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        held.append(p)
        return p.value

    def untouched():
        torch.cuda.synchronize()
        return bool((arena == 0x5a).all())
    try:
        for case in cases:
            RF.check(art, backend.lib, frame, case, base, host=host.ctypes.data, short=short)
            assert untouched(), case["name"]
    finally:
        torch.cuda.synchronize()
        for p in held:
            hip.hipFree(p)
    for case in (dict(name="good"), dict(name="in place", args={"out3f": "is color3f", "moments_out2f": "is moments2f"})):
        arena.fill_(0x5a)
        rc, text = RF.call(art, backend.lib, frame, case, base)
        torch.cuda.synchronize()
        assert rc == 0, (case["name"], text)
        # (the sentinel's frame is one of equal keys: nothing is clamped and out3f is the colour's own bytes; the flags are all 0)
        assert bool((arena[offsets["clamped1b"]:offsets["clamped1b"] + sizes["clamped1b"]] == 0).all()), case["name"]
    # and from Python: the library's refusals as ArtError
    W, H = frame
    c = torch.zeros((H, W, 3), device="cuda")
    with pytest.raises(art.ArtError, match="art_firefly_device: rank must be 1 .. 4"):
        backend.firefly_torch(c, rank=5)
    with pytest.raises(art.ArtError, match="art_firefly_device: an output overlaps an input plane"):
        big = torch.zeros(((H + 1) * W * 3,), device="cuda")                  # out3f one pixel into color3f
        backend.firefly_torch(big[:H * W * 3].view(H, W, 3), out=big[3:3 + H * W * 3].view(H, W, 3))


def gpu_temporal(backend, color, moments, n_colours, cam, cam_prev=None, hist=None, normal=None, depth=None, ids=None, scale=1.0, **kw):
    """temporal_ref.temporal's signature through Backend.temporal_torch: (history, out, variance, length) as numpy"""
    cur = dict(color=dev(color), moments=dev(moments), normal=dev(normal), depth=dev(depth), prim_index=dev(ids))
    out, var, length, new = backend.temporal_torch(cur, dev(hist), cam, cam_prev, n_colours, scale=scale, **kw)
    torch.cuda.synchronize()
    return new.cpu().numpy(), out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy()


def render_frames(art, backend, spp, frames=FQ.FRAMES):
    """the pan on the GPU: per frame (accum, moments, guides) as numpy, the render pass with accum and moments bound"""
    accum = torch.zeros((FQ.H, FQ.W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((FQ.H, FQ.W, 2), dtype=torch.float32, device="cuda")
    res = []
    try:
        backend.upload_scene(FQ.scene(0))
        backend.bind_accum(accum)
        backend.bind_moments(moments)
        for k in range(frames):
            p = art.Backend.pass_params(art.PT_MIS, False, FQ.DEPTH, spp, seed=FQ.SEED + k)
            backend.set_camera(*FQ.camera(k))
            backend.resize(FQ.W, FQ.H)
            got = backend.render_pass_device(p, 0)
            aovs = backend.render_aovs_torch(p, want=("normal", "depth", "prim_index"))
            torch.cuda.synchronize()
            assert got == spp
            res.append((accum.cpu().numpy().copy(), moments.cpu().numpy().copy(), {n: v.cpu().numpy() for n, v in aovs.items()}))
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)
    return res


_own = {}


def own_frames(art, backend):
    """the GPU's own four frames at the asserted spp, once per process"""
    if "f" not in _own:
        _own["f"] = render_frames(art, backend, FQ.ASSERTED_SPP)
    return _own["f"]


def test_end_to_end_pass_firefly_temporal(art, backend):
    """two frames of the pan at 48 x 48: the render pass with accum and moments bound, firefly_torch on the bound tensors as they are
    (scale = 1 / spp, ids from the feature buffers), temporal_torch with scale 1 -- everything on the GPU -- equals the references fed the
    same planes on every history word.  A setting that does clamp (gain 2) so that the moments rule is in the chain."""
    spp = FQ.ASSERTED_SPP
    setting = dict(radius=1, rank=2, gain=2.0, floor=0.0)
    accum = torch.zeros((FQ.H, FQ.W, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros((FQ.H, FQ.W, 2), dtype=torch.float32, device="cuda")
    h_gpu, h_ref, prev, clamped = None, None, None, 0
    try:
        backend.upload_scene(FQ.scene(0))
        backend.bind_accum(accum)
        backend.bind_moments(moments)
        for k in range(2):
            p = art.Backend.pass_params(art.PT_MIS, False, FQ.DEPTH, spp, seed=FQ.SEED + k)
            backend.set_camera(*FQ.camera(k))
            backend.resize(FQ.W, FQ.H)
            assert backend.render_pass_device(p, 0) == spp
            aovs = backend.render_aovs_torch(p, want=("normal", "depth", "prim_index"))
            out, mo, flags = backend.firefly_torch(accum, moments, aovs["prim_index"], scale=1.0 / spp, **setting)
            res = backend.temporal_torch(dict(aovs, color=out, moments=mo), h_gpu, FQ.camera(k), prev, spp, scale=1.0)
            torch.cuda.synchronize()
            hst = {n: v.cpu().numpy() for n, v in aovs.items()}
            rf = R.firefly(accum.cpu().numpy(), moments.cpu().numpy(), hst["prim_index"], scale=1.0 / spp, **setting)
            assert R.differ_all((out.cpu().numpy(), mo.cpu().numpy(), flags.cpu().numpy()), rf) == 0, "frame %d" % k
            r = T.temporal(rf[0], rf[1], spp, FQ.camera(k), cam_prev=prev, hist=h_ref, normal=hst["normal"], depth=hst["depth"], ids=hst["prim_index"],
                           max_history=art.TEMPORAL_MAX_HISTORY, depth_tol=art.TEMPORAL_DEPTH_TOL, normal_min=art.TEMPORAL_NORMAL_MIN, scale=1.0)
            assert all(T.differ(a.cpu().numpy(), b) == 0 for a, b in zip((res[3], res[0], res[1], res[2]), r)), "frame %d" % k
            clamped += int((rf[2] == 1).sum())
            h_gpu, h_ref, prev = res[3], r[0], FQ.camera(k)
        assert clamped > 0
    finally:
        torch.cuda.synchronize()
        backend.bind_moments(None)
        backend.bind_accum(None)


def test_planted_spikes_on_the_gpus_own_frame(art, backend):
    acc, mom, _ = own_frames(art, backend)[FQ.LAST]
    scale = 1.0 / FQ.ASSERTED_SPP
    got = FQ.check_planted(lambda c, m, i, **kw: gpu_firefly(backend, c, m, i, **kw), acc, mom, scale)
    pc, pm, _ = FQ.plant(acc, mom, scale)
    assert R.differ_all(got, R.firefly(pc, pm, None, scale=scale, **FQ.PLANT_SETTING)) == 0


def test_the_price_of_the_clamp_on_the_gpus_own_frames(art, backend):
    """tests/test_firefly_quality.py's assertion with both calls on the GPU over the GPU's own four frames (the sweep found no gain on
    this scene: what is asserted is the mean-luminance change, within 1.5 times the measured value)"""
    import test_firefly_quality as TQ
    TQ.price_of_the_clamp(art, lambda c, m, i, **kw: gpu_firefly(backend, c, m, i, **kw),
                          lambda *a, **kw: gpu_temporal(backend, *a, **kw), own_frames(art, backend))
