"""The tile deal of the sharded render (csrc/art_host_scene.cpp build_pixmap, through tests/host_sim) against the per-pixel numpy
reference written from the header's sentence (tests/pixmap_ref.py): every rank's pixel set, the partition of the frame, and the index
list itself -- in range, no pixel twice.  Rank counts on every branch of the skew rule (3; 5 when 3 divides n: 3, 6, 9; 7 when 15
divides n: 15), tiles of 1, 16 and 32 pixels, frames smaller than a tile, with partial tiles on one edge or both, and with more ranks
than tiles.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import hostsim
import pixmap_ref

RANKS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16)
TILES = (1, 16, 32)
FRAMES = ((1, 1), (33, 16), (40, 40), (70, 45), (96, 64), (257, 129))


def product_pixmap(art, w, h, rank, n, tile):
    """(the count hs_pixmap returns, the indices it wrote): the buffer has room to spare, so a list that is too long is seen, not cut"""
    L = hostsim.lib(art)
    L.hs_pixmap.restype = C.c_longlong
    L.hs_pixmap.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_longlong]
    out = np.full(w * h + 64, 0xFFFFFFFF, np.uint32)
    count = L.hs_pixmap(w, h, rank, n, tile, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size)
    return count, out[:max(0, min(count, out.size))].copy()


def test_the_skew_rule_of_the_header():
    assert [pixmap_ref.skew(n) for n in RANKS] == [3, 3, 5, 3, 3, 5, 3, 3, 5, 7, 3]
    assert pixmap_ref.skew(30) == 7 and pixmap_ref.skew(12) == 5 and pixmap_ref.skew(10) == 3
    for n in RANKS:                                      # odd and coprime to n: a row of tiles never repeats the row above
        assert np.gcd(pixmap_ref.skew(n), n) == 1


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("n", RANKS)
def test_product_deal_is_the_reference_deal(art, n, tile, frame):
    W, H = frame
    owners = pixmap_ref.owner_map(W, H, n, tile)
    seen = np.zeros(W * H, np.int64)
    for rank in range(n):
        count, pm = product_pixmap(art, W, H, rank, n, tile)
        mask = pixmap_ref.owner_mask(W, H, rank, n, tile)
        assert np.array_equal(mask, owners == rank)
        assert 0 <= count <= W * H and count == pm.size
        assert pm.size == 0 or int(pm.max()) < W * H, "rank %d: pixel index out of range" % rank
        assert np.unique(pm).size == pm.size, "rank %d: a pixel is listed twice" % rank
        got = np.zeros(W * H, bool)
        got[pm] = True
        assert np.array_equal(got.reshape(H, W), mask), "rank %d of %d, tile %d: %d pixels, the reference owns %d" % (rank, n, tile, pm.size, int(mask.sum()))
        seen[pm] += 1
    assert np.array_equal(seen, np.ones(W * H, np.int64)), "the ranks do not partition the frame"


@pytest.mark.parametrize("n,tile,frame", pixmap_ref.SHARD_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_reference_partitions_the_frames_of_the_gpu_tests(n, tile, frame):
    """The reference alone, on every (ranks, tile, frame) the GPU tests hand it: each pixel has exactly one owner among 0 .. n - 1, so
    what those tests assert per rank (zero outside the mask, the frame inside) adds up to the whole frame."""
    W, H = frame
    masks = np.stack([pixmap_ref.owner_mask(W, H, r, n, tile) for r in range(n)])
    assert masks.shape == (n, H, W) and np.array_equal(masks.sum(0), np.ones((H, W), np.int64))
    owners = pixmap_ref.owner_map(W, H, n, tile)
    assert owners.min() >= 0 and owners.max() < n
    # a tile is one rank's: constant on every tile x tile block, partial edge blocks included
    for y0 in range(0, H, tile):
        for x0 in range(0, W, tile):
            assert np.unique(owners[y0:y0 + tile, x0:x0 + tile]).size == 1


def test_ranks_without_a_tile():
    """40x40 in tiles of 32 is four tiles: (0,0) -> 0, (1,0) -> 1, (0,1) -> 3, (1,1) -> 4 of 8 ranks; 2, 5, 6 and 7 own nothing"""
    empty = [r for r in range(8) if not pixmap_ref.owner_mask(40, 40, r, 8, 32).any()]
    assert empty == [2, 5, 6, 7]
    assert [int(pixmap_ref.owner_mask(40, 40, r, 8, 32).sum()) for r in (0, 1, 3, 4)] == [32 * 32, 8 * 32, 32 * 8, 8 * 8]
