"""art_denoise_device on the GPU against the numpy reference written from the header (tests/denoise_ref.py): bit equality on small frames,
in place, non-finite input, stream order, refusals, end to end behind a render pass and the feature buffers, and without a scene."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
F = np.float32

# 64 x 4, 65 x 4 and 63 x 3 straddle a wave; 300 x 5 has rows longer than a workgroup's 256 pixels.  (One kernel exists, every tap from
# global memory: there is no tile whose edges would need sizes of their own.)
GPU_SIZES = R.SIZES + [(64, 4), (65, 4), (63, 3), (300, 5)]


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, F)).cuda()


def run(backend, color, g, kw, **more):
    out = backend.denoise_torch(dev(color), **{k: dev(v) for k, v in g.items()}, **kw, **more)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1: kernel against reference
@pytest.mark.parametrize("W,H", GPU_SIZES, ids=["%dx%d" % s for s in GPU_SIZES])
def test_kernel_equals_the_reference_bit_for_bit(backend, W, H):
    """192 parameter sets per size (denoise_ref.combos), each with variant 0, 1 and 2"""
    pl = R.planes(W, H)
    d_color, d_planes = dev(pl[0]), dict(zip(("albedo", "normal", "depth"), (dev(x) for x in pl[1:])))
    for c in R.combos():
        color, g, kw = R.combo_args(pl, c)
        want = R.denoise(color, **g, **kw)
        dg = {k: (d_planes[k] if v is not None else None) for k, v in g.items()}
        for variant in (0, 1, 2):
            got = backend.denoise_torch(d_color, **dg, **kw, variant=variant).cpu().numpy()
            assert got.shape == (H, W, 3) and R.differ(got, want) == 0, (R.combo_id(c), variant)


def test_eight_iterations_where_every_far_tap_is_off_image(backend):
    color, albedo, normal, depth = R.planes(37, 23)
    g, kw = dict(albedo=albedo, normal=normal, depth=depth), dict(iterations=8, scale=0.25)
    assert R.differ(run(backend, color, g, kw), R.denoise(color, **g, **kw)) == 0


# ------------------------------------------------------------------------------------------------ 2: in place
def test_in_place_gives_the_words_of_the_out_of_place_call(backend):
    color, albedo, normal, depth = R.planes(65, 9)
    d = [dev(x) for x in (color, albedo, normal, depth)]
    for it in (1, 2, 5):
        apart = backend.denoise_torch(*d, iterations=it, scale=0.5)
        same = d[0].clone()
        ret = backend.denoise_torch(same, *d[1:], iterations=it, scale=0.5, out=same)
        assert ret is same and torch.equal(apart.view(torch.int32), same.view(torch.int32))
        assert R.differ(apart.cpu().numpy(), R.denoise(color, albedo, normal, depth, iterations=it, scale=0.5)) == 0


# ------------------------------------------------------------------------------------------------ 3: non-finite input
def test_non_finite_input_against_the_reference_and_repair(backend):
    W, H = 21, 13
    color, albedo, normal, depth = R.planes(W, H)
    normal[:] = (0, 0, 1)
    clean = color.copy()
    color[6, 10] = (np.nan, 1.0, 1.0); color[2, 3] = (1.0, np.inf, 1.0); color[11, 18] = (-np.inf, 0.0, np.nan)
    normal[9, 4] = (np.nan, 0.0, 1.0); depth[4, 15] = np.nan; depth[0, 0] = np.inf
    g = dict(albedo=albedo, normal=normal, depth=depth)
    for it, sc in ((1, 0.0), (3, 4.0), (5, 0.0)):
        kw = dict(iterations=it, sigma_color=sc, scale=0.25)
        got = run(backend, color, g, kw)
        assert R.differ(got, R.denoise(color, **g, **kw)) == 0, (it, sc)
        assert np.isfinite(got).all()              # every bad colour pixel has good neighbours in reach: repaired, and nothing spread
    # after one iteration the output equals the clean image's at every pixel whose 5 x 5 taps hold none of the three bad colours
    kw = dict(iterations=1, sigma_color=0.0, scale=0.25)
    a, b = run(backend, clean, g, kw), run(backend, color, g, kw)
    yy, xx = np.mgrid[0:H, 0:W]
    untouched = np.ones((H, W), bool)
    for (y, x) in ((6, 10), (2, 3), (11, 18)):
        untouched &= (np.abs(yy - y) > 2) | (np.abs(xx - x) > 2)
    assert R.differ(a[untouched], b[untouched]) == 0 and untouched.sum() > 100
    one = np.full((1, 1, 3), np.nan, F)
    assert np.isnan(run(backend, one, {}, dict(iterations=2))).all()       # every tap skipped: the pixel keeps its value


# ------------------------------------------------------------------------------------------------ 4: stream order
def test_stream_order_on_a_side_stream(backend):
    W, H = 65, 33
    color, albedo, normal, depth = R.planes(W, H)
    src, d_alb, d_nrm, d_dep = (dev(x) for x in (color, albedo, normal, depth))
    d_color = torch.zeros_like(src)
    ballast = torch.empty(64 << 20, dtype=torch.float32, device="cuda")      # 256 MB: its fill keeps the stream busy in front of the copy
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ballast.fill_(1.0)
        d_color.copy_(src)                                           # the input is written by a torch op on the side stream ...
        out = backend.denoise_torch(d_color, d_alb, d_nrm, d_dep, iterations=3, scale=0.25)      # ... and read with no synchronisation between
        after = out * 2.0                                            # a torch op enqueued afterwards reads the finished output
    side.synchronize()
    want = R.denoise(color, albedo, normal, depth, iterations=3, scale=0.25)
    assert R.differ(out.cpu().numpy(), want) == 0
    assert R.differ(after.cpu().numpy(), want * F(2.0)) == 0


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals_at_the_c_level_leave_out_untouched(art, backend):
    W, H = 41, 25                                                    # N - 1 = 1024 pixels: the short planes below are whole 4 KiB pages
    N = W * H
    L = backend.lib
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    color, albedo, normal, depth = (dev(x) for x in R.planes(W, H))
    out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    host3, host1 = torch.zeros((H, W, 3), dtype=torch.float32), torch.zeros((H, W), dtype=torch.float32)

    def params(**kw):
        d = dict(width=W, height=H, iterations=2, demodulate=1, normal_log2=7, variant=0, scale=1.0, sigma_color=4.0, sigma_depth=1.0)
        d.update(kw)
        return art.ArtDenoiseParams(**d)

    def refused(p, ptrs, needle):
        rc = L.art_denoise_device(C.byref(p) if p is not None else None, *ptrs, None)
        assert rc != 0 and needle in L.art_last_error().decode(), (needle, L.art_last_error().decode())

    good = [color.data_ptr(), albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), out.data_ptr()]
    names = ("color3f", "albedo3f", "normal3f", "depth", "out3f")
    for k, name in enumerate(names):                                 # host memory for each pointer
        ptrs = list(good); ptrs[k] = (host1 if name == "depth" else host3).data_ptr()
        refused(params(), ptrs, name + " is not device memory")
    for k, name in enumerate(names):                                 # a plane too small by one pixel
        short = C.c_void_p(None)
        assert hip.hipMalloc(C.byref(short), (N - 1) * (4 if name == "depth" else 12)) == 0
        try:
            ptrs = list(good); ptrs[k] = short.value
            refused(params(), ptrs, name + " is smaller than")
        finally:
            hip.hipFree(short)
    refused(params(iterations=0), good, "iterations"); refused(params(iterations=9), good, "iterations")
    refused(params(normal_log2=11), good, "normal_log2"); refused(params(normal_log2=-1), good, "normal_log2")
    refused(params(variant=3), good, "variant")
    refused(params(scale=float("nan")), good, "scale"); refused(params(scale=float("inf")), good, "scale")
    refused(params(sigma_color=float("nan")), good, "sigma"); refused(params(sigma_depth=float("nan")), good, "sigma")
    refused(params(width=0), good, "width"); refused(params(height=0), good, "width"); refused(params(width=1 << 15, height=1 << 14), good, "width")
    refused(None, good, "null ArtDenoiseParams")
    refused(params(), [None] + good[1:], "null color3f or out3f"); refused(params(), good[:4] + [None], "null color3f or out3f")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert L.art_denoise_device(C.byref(params()), *good, None) == 0           # and the same arguments, unbroken, are accepted
    torch.cuda.synchronize(); backend.synchronize()
    assert not bool((out == 7.0).all())


def test_refusals_at_the_python_level_leave_out_untouched(art, backend):
    W, H = 9, 7
    color, albedo, normal, depth = (dev(x) for x in R.planes(W, H))
    out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    bad = [dict(color=color.double()), dict(albedo=albedo.half()), dict(depth=depth.int()),                     # a wrong dtype
           dict(color=color[:, :-1].contiguous()), dict(normal=normal[:-1].contiguous()), dict(depth=depth[..., None].contiguous()),
           dict(color=depth), dict(out=torch.empty((H, W), dtype=torch.float32, device="cuda")),                # a wrong shape
           dict(color=torch.zeros((H, 3, W), device="cuda").permute(0, 2, 1)), dict(depth=torch.zeros((W, H), device="cuda").t()),      # not contiguous
           dict(color=color.cpu()), dict(normal=normal.cpu()), dict(out=torch.zeros((H, W, 3))),                 # a CPU tensor
           dict(color=color.cpu().numpy()), dict(albedo=[1.0])]                                                  # not a tensor
    for change in bad:
        kw = dict(color=color, albedo=albedo, normal=normal, depth=depth, out=out)
        kw.update(change)
        with pytest.raises(art.ArtError):
            backend.denoise_torch(**kw)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 6: end to end
def test_end_to_end_behind_a_pass_and_the_feature_buffers(art, backend):
    """bind_accum + one PT_MIS pass (4 spp with AA) + render_aovs_torch + denoise_torch: the output is the reference on the downloaded
    planes; the accum tensor, stats() and stage_stats() are the same bytes before and after the call; and a following pass adds into the
    accum as if the call had not happened."""
    from ada_ray_tracer_amd import scenes
    W = H = 48
    sd = scenes.synthetic_scene(2000, 3)
    p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=7)

    def frame(with_denoise):
        accum = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        backend.upload_scene(sd)
        backend.bind_accum(accum)
        try:
            backend.resize(W, H)
            spp = backend.render_pass_device(p, 0)
            assert spp == 4
            seen = None
            if with_denoise:
                aovs = backend.render_aovs_torch(p)
                backend.synchronize(); torch.cuda.synchronize()
                before = (accum.clone(), bytes(backend.stats()), bytes(backend.stage_stats()))
                out = backend.denoise_torch(accum, **aovs, scale=1.0 / spp)
                backend.synchronize(); torch.cuda.synchronize()
                assert torch.equal(before[0].view(torch.int32), accum.view(torch.int32))
                assert before[1] == bytes(backend.stats()) and before[2] == bytes(backend.stage_stats())
                seen = (out.cpu().numpy(), accum.cpu().numpy(), {k: v.cpu().numpy() for k, v in aovs.items()})
            spp = backend.render_pass_device(p, spp)
            backend.synchronize(); torch.cuda.synchronize()
            st = backend.stats()
            return accum.cpu().numpy(), spp, (st.rays, st.samples, st.trace_launches), seen
        finally:
            backend.bind_accum(None)

    plain = frame(False)
    with_call = frame(True)
    out, acc4, a = with_call[3]
    want = R.denoise(acc4, a["albedo"], a["normal"], a["depth"], scale=1.0 / 4)
    assert R.differ(out, want) == 0
    assert np.isfinite(out).all() and np.abs(out - acc4 * F(0.25)).max() > 0          # (it did filter)
    assert plain[1] == with_call[1] == 8 and plain[2] == with_call[2]
    assert np.array_equal(plain[0].view(np.uint32), with_call[0].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 7: no scene needed
def test_no_scene_and_no_viewport_are_needed(art):
    """in a process of its own: art_init only, no upload, no resize"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, torch, __graft_entry__ as g, denoise_ref as R\n"
            "art = g.load_package(); be = art.Backend(0)\n"
            "color, albedo, normal, depth = R.planes(37, 23)\n"
            "d = [torch.from_numpy(x).cuda() for x in (color, albedo, normal, depth)]\n"
            "out = be.denoise_torch(*d, iterations=3, scale=0.5).cpu().numpy()\n"
            "print('DIFFER', R.differ(out, R.denoise(color, albedo, normal, depth, iterations=3, scale=0.5)))\n"
            "be.shutdown()\n") % (art.ROOT, os.path.join(art.ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DIFFER 0" in r.stdout, (r.stdout, r.stderr[-2000:])
