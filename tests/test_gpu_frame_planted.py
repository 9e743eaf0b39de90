"""The frame entries on framebuffers no path tracer produces.  art_bind_accum lets the caller own the framebuffer and art_download resolves
whatever lies in it, so a test can plant the words: the edge list of the resolve known-answer op (tests/kat_inputs.py resolve_case: +-0,
denormals, negative sums, NaN, +-inf, sums far above 1, and for every byte the sum at which it rises, one ulp below and one above), tiled
over the frame, and an index-coded plane in which every word is distinct, a third of them NaNs with payloads of their own.

Expected, all compared as uint32 words without a tolerance:
  * the accum copy is the planted words, in LAYOUT_ADA_XY their transpose (k_to_xmajor_f3), NaN payloads included;
  * the screen is orc.resolve(planted, spp), in LAYOUT_ADA_XY its transpose (k_resolve, k_to_xmajor_u32), for spp 1, 3, 7 and 256;
  * the bound tensor still holds what was planted.
The frames put one pixel short of, exactly at and one past a workgroup of 256 (255x1, 16x16, 257x1) and are not square (1x7, 7x1, 67x5,
5x67, 257x3): where x / h written for x / w, or a guard off by one, shows.  Then the rule of include/art_hip.h for spp <= 0, one debug pass
and one render pass on non-square frames."""
import ctypes as C

import numpy as np
import pytest
import torch

import kat_inputs as ki
import orc
import test_gpu_bound_accum as ba          # restore, words
import test_gpu_shade_per as sp            # scene, SEED

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (1, 7), (7, 1), (16, 16), (255, 1), (257, 1), (67, 5), (5, 67), (257, 3)]
SPPS = [1, 3, 7, 256]
SENTINEL = 0xA5A5A5A5
ids = lambda f: "%dx%d" % f


def index_plane(W, H):
    """[H, W, 3] words, every one distinct: word j of the frame is j + 1 (a denormal), a quiet NaN with payload j, or a negative
    signalling NaN with payload j + 1, by pixel mod 3"""
    j = np.arange(3 * W * H, dtype=np.uint32).reshape(H * W, 3)
    kind = (np.arange(H * W) % 3)[:, None]
    w = np.where(kind == 0, j + 1, np.where(kind == 1, np.uint32(0x7FC00000) | j, np.uint32(0xFF800001) + j)).astype(np.uint32)
    assert np.unique(w).size == w.size
    return w.reshape(H, W, 3)


def resolve_plane(W, H, spp):
    """the edge items of the resolve op that belong to spp, tiled over the frame from an offset of the frame's own"""
    case, = ki.cases("resolve")
    e = case.words[:case.n_edge]
    rows = e[e[:, 3] == (np.float32(1) / np.float32(spp)).view(np.uint32), :3]
    assert rows.shape[0] >= 3 * 255
    return np.ascontiguousarray(rows[(np.arange(W * H) + 31 * W + H) % rows.shape[0]]).reshape(H, W, 3)


def planes(W, H):
    return [("index", index_plane(W, H))] + [("resolve inputs of spp %d" % s, resolve_plane(W, H, s)) for s in SPPS]


def plant(t, words):
    """the words into the tensor as they are: an integer copy, no float operation sees them"""
    t.view(torch.int32)[:words.size].copy_(torch.from_numpy(np.ascontiguousarray(words).reshape(-1).view(np.int32)))
    torch.cuda.synchronize()


def download(art, backend, layout, spp, want_accum, want_screen):
    """art_download with either pointer NULL; the buffers start as SENTINEL.  Returns (rc, accum words or None, screen or None)"""
    shape = backend._frame_shape(layout)
    accum = np.full(shape + (3,), SENTINEL, np.uint32) if want_accum else None
    screen = np.full(shape, SENTINEL, np.uint32) if want_screen else None
    rc = backend.lib.art_download(accum.ctypes.data_as(C.POINTER(C.c_float)) if want_accum else None,
                                  screen.ctypes.data_as(C.POINTER(C.c_uint32)) if want_screen else None, layout, spp)
    return rc, accum, screen


def bound(backend, W, H):
    """a zero tensor of the frame's size, bound, and the frame set"""
    t = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    backend.bind_accum(t)
    backend.resize(W, H)
    return t


@pytest.mark.parametrize("frame", FRAMES, ids=ids)
def test_downloads_of_a_planted_framebuffer(art, backend, frame):
    W, H = frame
    ba.restore(backend)
    try:
        backend.upload_scene(sp.scene(art, "synthetic")[0])
        t = bound(backend, W, H)
        assert not ba.words(t, W, H).any()
        for name, p in planes(W, H):
            plant(t, p)
            want_screen = {spp: orc.resolve(p.view(np.float32), spp) for spp in SPPS}
            for layout, tr3, tr2 in ((art.LAYOUT_ROW_MAJOR, lambda a: a, lambda a: a), (art.LAYOUT_ADA_XY, lambda a: a.transpose(1, 0, 2), lambda a: a.T)):
                what = "%s, layout %d" % (name, layout)
                for spp in SPPS + [0, -3]:                                       # the accum alone: spp is not read
                    rc, acc, _ = download(art, backend, layout, spp, True, False)
                    assert rc == 0, backend.lib.art_last_error().decode()
                    assert np.array_equal(acc, tr3(p)), "%s: the accum copy is not the planted words: %s" % (what, ba.differ(acc, tr3(p)))
                for spp in SPPS:
                    rc, _, scr = download(art, backend, layout, spp, False, True)
                    assert rc == 0, backend.lib.art_last_error().decode()
                    assert np.array_equal(scr, tr2(want_screen[spp])), "%s, spp %d, the screen alone: %s" % (what, spp, ba.differ(scr, tr2(want_screen[spp])))
                    rc, acc, scr = download(art, backend, layout, spp, True, True)
                    assert rc == 0, backend.lib.art_last_error().decode()
                    assert np.array_equal(acc, tr3(p)), "%s, spp %d, both: the accum: %s" % (what, spp, ba.differ(acc, tr3(p)))
                    assert np.array_equal(scr, tr2(want_screen[spp])), "%s, spp %d, both: the screen: %s" % (what, spp, ba.differ(scr, tr2(want_screen[spp])))
            got = ba.words(t, W, H)
            assert np.array_equal(got, p), "%s: the downloads changed the bound tensor: %s" % (name, ba.differ(got, p))
    finally:
        ba.restore(backend)


@pytest.mark.parametrize("frame", [(67, 5), (257, 1)], ids=ids)
def test_a_screen_needs_a_positive_spp(art, backend, frame):
    """include/art_hip.h, art_download: with a screen asked for, spp <= 0 is refused before any launch -- the error names spp, the host
    buffers and the bound tensor keep their words -- and the next good call works; the accum alone comes back with any spp."""
    W, H = frame
    ba.restore(backend)
    try:
        backend.upload_scene(sp.scene(art, "synthetic")[0])
        t = bound(backend, W, H)
        p = index_plane(W, H)
        plant(t, p)
        for layout in (art.LAYOUT_ROW_MAJOR, art.LAYOUT_ADA_XY):
            for spp in (0, -1, -256, -(1 << 31)):
                for want_accum in (False, True):
                    rc, acc, scr = download(art, backend, layout, spp, want_accum, True)
                    err = backend.lib.art_last_error().decode()
                    assert rc != 0 and "art_download" in err and "spp" in err, (rc, err)
                    assert (scr == SENTINEL).all() and (acc is None or (acc == SENTINEL).all()), "a refused download wrote to a host buffer"
                    assert np.array_equal(ba.words(t, W, H), p), "a refused download changed the bound tensor"
                rc, acc, _ = download(art, backend, layout, spp, True, False)
                assert rc == 0, backend.lib.art_last_error().decode()
                assert np.array_equal(acc, p if layout == art.LAYOUT_ROW_MAJOR else p.transpose(1, 0, 2))
            rc, acc, scr = download(art, backend, layout, 3, True, True)
            assert rc == 0 and np.array_equal(scr, orc.resolve(p.view(np.float32), 3) if layout == art.LAYOUT_ROW_MAJOR else orc.resolve(p.view(np.float32), 3).T)
        with pytest.raises(art.ArtError, match="spp"):
            backend.download(0, art.LAYOUT_ROW_MAJOR)
    finally:
        ba.restore(backend)


def test_the_debug_pass_resolves_what_it_returns(art, backend):
    """art_debug_hit_pass into the bound tensor on 67x5, both layouts: the screen it returns is orc.resolve (spp 1) of the accum it returns,
    and the tensor holds that accum, row-major"""
    W, H = 67, 5
    ba.restore(backend)
    try:
        backend.upload_scene(sp.scene(art, "synthetic")[0])
        t = bound(backend, W, H)
        for layout in (art.LAYOUT_ROW_MAJOR, art.LAYOUT_ADA_XY):
            plant(t, index_plane(W, H))                                      # a written image, not one added to what was there
            acc, screen, prim, _, _ = backend.debug_hit_pass(art.Backend.pass_params(art.RT_DEBUG, False, 8, 1, seed=sp.SEED, layout=layout))
            row = np.ascontiguousarray(acc if layout == art.LAYOUT_ROW_MAJOR else acc.transpose(1, 0, 2))
            assert row.shape == (H, W, 3) and row.any() and len(np.unique(prim)) > 1
            want = orc.resolve(row, 1)
            assert np.array_equal(screen, want if layout == art.LAYOUT_ROW_MAJOR else want.T), "layout %d: %s" % (layout, ba.differ(screen, want if layout == art.LAYOUT_ROW_MAJOR else want.T))
            assert np.array_equal(ba.words(t, W, H), row.view(np.uint32))
    finally:
        ba.restore(backend)


def test_a_tall_render_pass_in_the_ada_layout_is_the_oracles(art, backend):
    """one PT_MIS pass with host pointers on 5x67 in LAYOUT_ADA_XY: accum and screen are the oracle's, transposed"""
    W, H = 5, 67
    sd, osc, _ = sp.scene(art, "synthetic")
    ref, rspp, _ = orc.render(osc.scene, orc.make_params(W, H, orc.PT_MIS, True, 8, 1, seed=sp.SEED))
    ba.restore(backend)
    try:
        backend.upload_scene(sd)
        backend.resize(W, H)
        acc, screen, spp = backend.render_pass(art.Backend.pass_params(art.PT_MIS, True, 8, 1, seed=sp.SEED, layout=art.LAYOUT_ADA_XY), 0, True, True)
        assert spp == rspp == 4 and acc.shape == (W, H, 3) and screen.shape == (W, H) and ref.any()
        assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32).transpose(1, 0, 2)), ba.differ(acc.view(np.uint32), ref.view(np.uint32).transpose(1, 0, 2))
        assert np.array_equal(screen, orc.resolve(ref, spp).T)
    finally:
        ba.restore(backend)
