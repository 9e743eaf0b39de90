"""Adaptive sampling on the GPU: art_compact_mask_device against its numpy statement, art_render_pass_masked against the full pass on the
mask (words, not floats: NaNs and -0 count), art_adaptive_estimate_device against tests/adaptive_ref.py bit for bit, its variance plane
through the variance-guided filter, Backend.render_adaptive end to end with the CPU sweep's bound, and the refusals.

The rank's pixel list is written here from the header's sentences (tiles of 32 x 32 dealt by tests/pixmap_ref.py, tile after tile in
row-major tile order, rows inside a tile), not taken from the product.  The backend is the session's: every test ends in restore()."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

import adaptive_quality as Q
import adaptive_ref as R
import pixmap_ref
import test_gpu_bound_accum as ba
import test_gpu_moments as gm
import test_gpu_shade_per as sp

pytestmark = pytest.mark.gpu

F = np.float32
TILE = 32


def restore(backend):
    gm.restore(backend)


def pixel_list(W, H, rank=0, n=1, tile=TILE):
    own = pixmap_ref.owner_mask(W, H, rank, n, tile)
    ys, xs = np.nonzero(own)
    order = np.lexsort((xs, ys, xs // tile, ys // tile))          # tile row, tile column, then the rows of the tile
    return (ys[order] * W + xs[order]).astype(np.uint32)


def masks_of(W, H, pixmap, seed=1):
    """name -> [H, W] uint8"""
    rng = np.random.default_rng(seed)
    N = W * H
    one = lambda g: np.bincount([g], minlength=N).astype(np.uint8).reshape(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    tile = ((yy // TILE == (H - 1) // TILE) & (xx // TILE == min(1, (W - 1) // TILE))).astype(np.uint8)
    m = {"empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8), "checkerboard": ((xx + yy) & 1).astype(np.uint8), "tile": tile,
         "random30": (rng.random((H, W)) < 0.3).astype(np.uint8), "bytes": ((rng.random((H, W)) < 0.5) * rng.integers(2, 256, (H, W))).astype(np.uint8)}
    if len(pixmap):
        m["first"] = one(int(pixmap[0])); m["last"] = one(int(pixmap[-1]))
    return m


def gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def compacted(backend, mask):
    pixels, count = backend.compact_mask_torch(gpu(mask))
    torch.cuda.synchronize()
    return pixels.cpu().numpy().view(np.uint32), int(count.item())


# ---- compaction ------------------------------------------------------------------------------------------------------------------------
COMPACT_FRAMES = [(1, 1), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (1025, 1), (70, 50), (300, 300)]


def check_compaction(backend, W, H, rank, n):
    pixmap = pixel_list(W, H, rank, n)
    for name, mask in masks_of(W, H, pixmap).items():
        want = R.compact(mask, pixmap)
        got, count = compacted(backend, mask)
        assert count == len(want), "%s: count %d, expected %d" % (name, count, len(want))
        assert np.array_equal(got[:count], want), "%s: the list differs" % name
        again, count2 = compacted(backend, mask)
        assert count2 == count and np.array_equal(again[:count], got[:count]), "%s: two runs differ" % name


@pytest.mark.parametrize("frame", COMPACT_FRAMES, ids=lambda f: "%dx%d" % f)
def test_compaction_equals_numpy(backend, frame):
    W, H = frame
    try:
        backend.resize(W, H)
        assert (W, H) != (300, 300) or (W * H + 255) // 256 == 352          # more workgroups than one step of the block scan holds
        check_compaction(backend, W, H, 0, 1)
    finally:
        restore(backend)


@pytest.mark.parametrize("rank", [1, 2])
def test_compaction_of_a_shard(backend, rank):
    W, H = 70, 50
    try:
        backend.set_shard(rank, 3, TILE)
        backend.resize(W, H)
        assert 0 < len(pixel_list(W, H, rank, 3)) < W * H
        check_compaction(backend, W, H, rank, 3)
    finally:
        restore(backend)


def test_compaction_writes_nothing_past_the_count_and_checks_cap(backend):
    W, H = 70, 50
    L = backend.lib
    try:
        backend.resize(W, H)
        pixmap = pixel_list(W, H)
        mask = masks_of(W, H, pixmap)["random30"]
        out = torch.full((W * H + 7,), -1, dtype=torch.int32, device="cuda")
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        assert L.art_compact_mask_device(gpu(mask).data_ptr(), out.data_ptr(), W * H + 7, count.data_ptr(), art_stream()) == 0
        torch.cuda.synchronize()
        k = int(count.item())
        assert k == int(mask.sum()) and bool((out[k:] == -1).all()) and np.array_equal(out[:k].cpu().numpy().view(np.uint32), R.compact(mask, pixmap))
        assert L.art_compact_mask_device(gpu(mask).data_ptr(), out.data_ptr(), W * H - 1, count.data_ptr(), art_stream()) != 0
        assert "cap" in L.art_last_error().decode()
        host = np.zeros(W * H, np.uint8)
        assert L.art_compact_mask_device(host.ctypes.data, out.data_ptr(), W * H, count.data_ptr(), art_stream()) != 0
        assert "mask1b is not device memory" in L.art_last_error().decode()
    finally:
        restore(backend)


def art_stream():
    return torch.cuda.current_stream().cuda_stream or 1       # hipStreamLegacy: torch's default stream is the null stream


# ---- the masked pass equals the full pass on the mask --------------------------------------------------------------------------------------
class Run:
    """accum, moments and counts tensors bound to the session's backend for one frame"""

    def __init__(self, art, backend, name, frame, shard=None, bind=True, upload=True):
        self.be, self.W, self.H, self.bind = backend, frame[0], frame[1], bind
        N = self.W * self.H
        self.t = torch.zeros(3 * N, dtype=torch.float32, device="cuda")
        self.m = torch.zeros(2 * N, dtype=torch.float32, device="cuda")
        self.counts = torch.zeros(N, dtype=torch.int32, device="cuda")
        if upload:
            backend.upload_scene(ba.scene(art, name))
        if bind:
            backend.bind_accum(self.t)
        backend.bind_moments(self.m)
        if shard:
            backend.set_shard(shard[0], shard[1], TILE)
        backend.resize(self.W, self.H)
        self.spp = 0

    def full(self, p):
        self.spp = self.be.render_pass_device(p, self.spp)

    def masked(self, p, mask, counts=True):
        self.spp, k = self.be.render_pass_masked(p, self.spp, gpu(mask), self.counts if counts else None)
        return k

    def words(self):
        """(accum [H, W, 3], moments [H, W, 2], counts [H, W]) as uint32 words"""
        torch.cuda.synchronize()
        N = self.W * self.H
        if self.bind:
            acc = self.t.cpu().numpy().view(np.uint32).reshape(self.H, self.W, 3).copy()
        else:
            acc = np.ascontiguousarray(self.be.download(1, want_screen=False)[0]).view(np.uint32).reshape(self.H, self.W, 3).copy()
        return acc, self.m.cpu().numpy().view(np.uint32).reshape(self.H, self.W, 2).copy(), self.counts.cpu().numpy().view(np.uint32).reshape(self.H, self.W).copy()


VARIANTS = {  # scene, aa, vthreads, batch_paths, shard, accum bound
    "flat-aa": ("synthetic", True, 1, None, None, True),
    "flat-noaa-v2": ("synthetic", False, 2, None, None, True),
    "instanced-aa-v2": ("instanced", True, 2, None, None, True),
    "instanced-noaa": ("instanced", False, 1, None, None, True),
    "flat-batches": ("synthetic", True, 2, 1024, None, True),
    "flat-shard": ("synthetic", True, 1, None, (1, 3), True),
    "flat-own-accum": ("synthetic", True, 1, None, None, False),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_masked_pass_equals_the_full_pass_on_the_mask(art, backend, variant):
    name, aa, vthreads, batch, shard, bind = VARIANTS[variant]
    frame = W, H = (70, 50)
    p = ba.params(art, "PT_MIS", aa, vthreads)
    S = vthreads * (4 if aa else 1)
    own = pixmap_ref.owner_mask(W, H, shard[0], shard[1], TILE) if shard else np.ones((H, W), bool)
    pixmap = pixel_list(W, H, *(shard or (0, 1)))
    if batch:
        backend.set_option("batch_paths", batch)
    try:
        b = Run(art, backend, name, frame, shard, bind)
        b.full(p)
        first = b.words()
        b.full(p)
        second, b_stats, b_spp = b.words(), backend.stats(), b.spp
        assert not np.array_equal(first[0], second[0])
        for mname, mask in masks_of(W, H, pixmap).items():
            if mname in ("checkerboard", "bytes", "last"):
                continue
            a = Run(art, backend, name, frame, shard, bind, upload=False)
            a.full(p)
            assert all(np.array_equal(x, y) for x, y in zip(a.words()[:2], first[:2])), mname
            k = a.masked(p, mask)
            got = a.words()
            M = (mask != 0) & own
            assert k == int(M.sum()) and a.spp == b_spp, mname
            for plane, g, on, off in zip(("accum", "moments"), got, second, first):
                assert np.array_equal(g[M], on[M]), "%s: %s on the mask is not the full pass's" % (mname, plane)
                assert np.array_equal(g[~M], off[~M]), "%s: %s off the mask was written" % (mname, plane)
            assert np.array_equal(got[2], np.where(M, S, 0).astype(np.uint32)), "%s: counts" % mname
            st = backend.stats()
            assert st.lost_paths == 0 and st.samples == (int(own.sum()) + k) * S
            if mname == "full":
                assert st.rays == b_stats.rays and st.samples == b_stats.samples
            if mname == "empty":
                assert k == 0 and all(np.array_equal(x, y) for x, y in zip(got[:2], first[:2]))
    finally:
        if batch:
            backend.set_option("batch_paths", sp.DEFAULT_BATCH_PATHS)
        restore(backend)


def test_later_passes_are_unaffected(art, backend):
    """full, masked M, full: off M the frame is full + a full pass entered with spp advanced by S (the skipped indices stay skipped); on M it
    is three full passes."""
    frame = W, H = (70, 50)
    p = ba.params(art, "PT_MIS", True, 1)
    mask = masks_of(W, H, pixel_list(W, H))["random30"]
    M = mask != 0
    try:
        a = Run(art, backend, "synthetic", frame)
        a.full(p); a.masked(p, mask, counts=False); a.full(p)
        got = a.words()
        assert backend.stats().lost_paths == 0 and a.spp == 12
        b = Run(art, backend, "synthetic", frame, upload=False)
        b.full(p); b.spp += 4; b.full(p)
        skipped = b.words()
        c = Run(art, backend, "synthetic", frame, upload=False)
        c.full(p); c.full(p); c.full(p)
        three = c.words()
        for k in (0, 1):
            assert np.array_equal(got[k][~M], skipped[k][~M]) and np.array_equal(got[k][M], three[k][M])
        assert not np.array_equal(skipped[0][M], three[0][M])
    finally:
        restore(backend)


# ---- the estimate kernel ---------------------------------------------------------------------------------------------------------------
def estimate_gpu(backend, accum, mom, counts, aa, **kw):
    out = backend.adaptive_estimate_torch(gpu(accum), gpu(mom), gpu(counts.view(np.int32)), aa, **kw)
    torch.cuda.synchronize()
    return [out[k].cpu().numpy() for k in ("mean", "variance", "error", "mask")]


def same_estimate(got, want):
    for name, g, w in zip(("mean", "variance", "error"), got, want):
        gw, ww = np.ascontiguousarray(g).view(np.uint32).reshape(-1), np.ascontiguousarray(w).view(np.uint32).reshape(-1)
        bad = np.flatnonzero(gw != ww)
        assert len(bad) == 0, "%s: %d words differ, the first at word %d: got %08x, expected %08x" % (name, len(bad), bad[0], gw[bad[0]], ww[bad[0]])
    assert np.array_equal(got[3], want[3]), "mask"


@pytest.mark.parametrize("lum_floor", [0.0, 0.01])
@pytest.mark.parametrize("aa", [False, True], ids=["noaa", "aa"])
def test_estimate_equals_the_reference_on_planted_planes(backend, aa, lum_floor):
    W, H, max_samples, min_colours = 70, 50, 96, 4
    try:
        backend.resize(W, H)
        accum, mom, counts, thr = R.planted(W, H, aa, max_samples, lum_floor)
        kw = dict(threshold=float(thr), lum_floor=lum_floor, min_colours=min_colours, max_samples=max_samples)
        got = estimate_gpu(backend, accum, mom, counts, aa, **kw)
        same_estimate(got, R.estimate(accum, mom, counts, aa, **kw))
        assert got[2].reshape(-1)[11] == thr and got[3].reshape(-1)[11] == 0 and got[3].reshape(-1)[0] == 1
        only = backend.adaptive_estimate_torch(gpu(accum), gpu(mom), gpu(counts.view(np.int32)), aa, want=("mask",), **kw)
        assert set(only) == {"mask"} and np.array_equal(only["mask"].cpu().numpy(), got[3])
    finally:
        restore(backend)


@pytest.fixture(scope="module")
def masked_run(art, backend):
    """planes a real masked run produced at 48 x 48 (the quality scene, no anti-aliasing): a full pass of 4 samples, then three masked
    passes of 4 steered by the estimate; host copies, and the frame's feature buffers"""
    W, H = Q.W, Q.H
    p = art.Backend.pass_params(art.PT_MIS, Q.AA, Q.DEPTH, 4, seed=Q.SEED)
    try:
        backend.upload_scene(Q.scene())
        t = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"); m = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
        counts = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        backend.bind_accum(t); backend.bind_moments(m)
        backend.resize(W, H)
        spp = backend.render_pass_device(p, 0)
        counts += spp
        for _ in range(3):
            mask = backend.adaptive_estimate_torch(t, m, counts, Q.AA, threshold=0.05, lum_floor=0.1, min_colours=8, want=("mask",))["mask"]
            spp, k = backend.render_pass_masked(p, spp, mask, counts)
        aovs = backend.render_aovs_torch(p, want=("albedo", "normal", "depth"))
        torch.cuda.synchronize()
        return dict(accum=t.cpu().numpy(), moments=m.cpu().numpy(), counts=counts.cpu().numpy().view(np.uint32), guides={n: v.cpu().numpy() for n, v in aovs.items()})
    finally:
        restore(backend)


def test_estimate_equals_the_reference_on_a_real_masked_run(backend, masked_run):
    r = masked_run
    assert len(np.unique(r["counts"])) > 2 and r["counts"].min() >= 4
    kw = dict(threshold=0.05, lum_floor=0.1, min_colours=8, max_samples=64)
    try:
        backend.resize(Q.W, Q.H)
        same_estimate(estimate_gpu(backend, r["accum"], r["moments"], r["counts"], Q.AA, **kw), R.estimate(r["accum"], r["moments"], r["counts"], Q.AA, **kw))
    finally:
        restore(backend)


def test_variance_plane_feeds_the_filter(art, backend, masked_run):
    """variance1f through denoise_svgf_torch(variance=) with scale = 1 equals the numpy reference of art_denoise_svgf_var_device on the same planes"""
    import svgf_var_ref as V
    import svgf_ref as S
    r = masked_run
    kw = dict(threshold=0.05, lum_floor=0.1, min_colours=8, max_samples=64)
    try:
        backend.resize(Q.W, Q.H)
        mean, var, _, _ = estimate_gpu(backend, r["accum"], r["moments"], r["counts"], Q.AA, **kw)
        assert np.isfinite(var).all() and (var > 0).any()
        vout = torch.empty((Q.H, Q.W), dtype=torch.float32, device="cuda")
        filt = backend.denoise_svgf_torch(gpu(mean), variance=gpu(var), variance_out=vout, scale=1.0, **{k: gpu(v) for k, v in r["guides"].items()})
        torch.cuda.synchronize()
        ref = V.denoise_var(mean, var, iterations=art.SVGF_ITERATIONS, sigma_color=art.SVGF_SIGMA_COLOR, **r["guides"])
        assert S.differ(filt.cpu().numpy(), ref[0]) == 0 and S.differ(vout.cpu().numpy(), ref[1]) == 0
    finally:
        restore(backend)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_render_adaptive_end_to_end(art, backend):
    W, H = Q.W, Q.H
    p = art.Backend.pass_params(art.PT_MIS, Q.AA, Q.DEPTH, 1, seed=Q.SEED)
    try:
        backend.upload_scene(Q.scene())
        backend.resize(W, H)
        res = backend.render_adaptive(p, Q.BUDGET, Q.STEP_VTHREADS, max_samples=Q.MAX_SAMPLES, first_vthreads=Q.FIRST_VTHREADS, max_passes=200)
        counts = res["counts"].cpu().numpy().astype(np.int64)
        assert 1 < res["passes"] < 200, "the loop did not end by itself"
        assert counts.sum() == res["samples"] <= Q.BUDGET and counts.max() <= Q.MAX_SAMPLES and counts.min() >= Q.FIRST_VTHREADS
        assert backend.stats().lost_paths == 0 and backend._accum_tensor is None and backend._moments_tensor is None
        mean = res["mean"].cpu().numpy()
        assert np.array_equal(mean, res["accum"].cpu().numpy() * (F(1.0) / counts.astype(F))[..., None])
        backend.resize(W, H)
        uni = art.Backend.pass_params(art.PT_MIS, Q.AA, Q.DEPTH, Q.BUDGET_SPP, seed=Q.SEED)
        acc, _, spp = backend.render_pass(uni, 0)
        assert spp == Q.BUDGET_SPP
        ref = Q.reference()
        uniform, adaptive = Q.rms(acc / F(spp), ref), Q.rms(mean, ref)
        bound = Q.bound(Q.shipped()["best"])
        print("RMS against 1024 spp: uniform %d spp %.5f, adaptive %.5f with %d of %d samples in %d passes; bound %.3f"
              % (spp, uniform, adaptive, res["samples"], Q.BUDGET, res["passes"], bound))
        assert adaptive < bound * uniform
    finally:
        restore(backend)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(art, backend):
    frame = W, H = (70, 50)
    N = W * H
    L = backend.lib
    p = ba.params(art, "PT_MIS", True, 1)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    mask = torch.ones(N, dtype=torch.uint8, device="cuda")
    short = C.c_void_p(None)
    assert hip.hipMalloc(C.byref(short), N - 1) == 0
    try:
        a = Run(art, backend, "synthetic", frame)
        a.full(p)
        a.counts.fill_(3)
        before = a.words()

        def refused(text, params=p, m=mask.data_ptr(), c=a.counts.data_ptr(), spp=4):
            s = C.c_int32(spp); k = C.c_int64(-5)
            assert L.art_render_pass_masked(C.byref(params), m, c, C.byref(s), C.byref(k)) != 0
            assert text in L.art_last_error().decode(), (text, L.art_last_error().decode())
            assert s.value == spp and k.value == -5 and all(np.array_equal(x, y) for x, y in zip(a.words(), before)), text
        refused("null mask1b", m=None)
        refused("mask1b is not device memory", m=np.ones(N, np.uint8).ctypes.data)
        refused("counts1u is not device memory", c=np.zeros(N, np.uint32).ctypes.data)
        refused("mask1b is smaller than", m=short.value)
        refused("counts1u is smaller than", c=short.value)
        refused("debug render types", params=art.Backend.pass_params(art.RT_DEBUG, False, 8, 1))
        refused("multiple of 4", spp=6)
        with pytest.raises(art.ArtError, match="mask: the tensor holds"):
            backend.render_pass_masked(p, 4, mask[:N - 1])
        with pytest.raises(art.ArtError, match="counts: dtype"):
            backend.render_pass_masked(p, 4, mask, torch.zeros(N, dtype=torch.float32, device="cuda"))
        # an instanced scene with the one-ray-per-lane schedule
        backend.upload_scene(ba.scene(art, "instanced"))
        backend.set_option("trace_kernel", 1)
        try:
            refused("an instanced scene renders through the record schedule only")
        finally:
            backend.set_option("trace_kernel", 0)
        # the call goes through afterwards
        backend.upload_scene(ba.scene(art, "synthetic"))
        s = C.c_int32(4)
        assert L.art_render_pass_masked(C.byref(p), mask.data_ptr(), a.counts.data_ptr(), C.byref(s), None) == 0 and s.value == 8
        assert bool((a.counts == 7).all())
    finally:
        hip.hipFree(short)
        restore(backend)


CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import __graft_entry__ as ge
art = ge.load_package()
from ada_ray_tracer_amd import scenes
L = art.load_library()
p = art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=7)
one = C.c_void_p(16)
s = C.c_int32(0)
print(L.art_render_pass_masked(C.byref(p), one, None, C.byref(s), None), L.art_last_error().decode())          # no scene
be = art.Backend(0)
be.upload_scene(scenes.synthetic_scene(2000, 3))
mask = torch.ones(48 * 48, dtype=torch.uint8, device="cuda")
print(L.art_render_pass_masked(C.byref(p), mask.data_ptr(), None, C.byref(s), None), L.art_last_error().decode())   # no resize
be.shutdown()
be = art.Backend(devices=[0, 0])
be.upload_scene(scenes.synthetic_scene(2000, 3)); be.resize(48, 48)
print(L.art_render_pass_masked(C.byref(p), mask.data_ptr(), None, C.byref(s), None), L.art_last_error().decode())   # two contexts
print(s.value)
be.shutdown()
"""


def test_refusals_without_scene_or_frame_and_with_two_contexts(art):
    """a process of its own: the session's backend has a scene and one context"""
    r = subprocess.run([sys.executable, "-c", CHILD, art.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.strip().split("\n")
    assert out[0].startswith("1 ") and "no scene" in out[0]
    assert out[1].startswith("1 ") and "no viewport" in out[1]
    assert out[2].startswith("1 ") and "art_render_pass_masked: not available after art_init_devices" in out[2]
    assert out[3] == "0"
