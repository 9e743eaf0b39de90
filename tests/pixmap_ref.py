"""Who owns a pixel: a numpy reference of the tile deal, written from the sentence in include/art_hip.h at art_init_devices --
"device k owns the pixel tiles (bx, by) with (bx + skew by) mod n == k (skew = 3, or 5 when 3 divides n, or 7 when 15 divides n)" --
with tile x tile pixel tiles counted from the frame's top left corner, the last column and row of tiles cut off at the frame's edge.
It is not a copy of the product's loop (csrc/art_host_scene.cpp build_pixmap): it works per pixel, the product per tile.

SHARD_CASES are the (ranks, tile, frame) combinations the GPU tests of the sharded render use (tests/test_gpu_bound_accum.py,
tests/test_gpu_parity.py); tests/test_pixmap.py checks, without a GPU, that the reference deals each of them as a partition."""
import numpy as np


def skew(n):
    return 7 if n % 15 == 0 else 5 if n % 3 == 0 else 3


def owner_map(W, H, n, tile):
    """[H, W] int64: the rank that owns pixel (x, y)"""
    bx = np.arange(W, dtype=np.int64) // tile
    by = np.arange(H, dtype=np.int64) // tile
    return (bx[None, :] + skew(n) * by[:, None]) % n


def owner_mask(W, H, rank, n, tile):
    """[H, W] bool: the pixels rank owns in an n-way job"""
    return owner_map(W, H, n, tile) == rank


SHARD_RANKS = (2, 3, 5, 8)
SHARD_TILES = (16, 32)
SHARD_FRAMES = ((70, 45), (40, 40))          # partial tiles on both edges; fewer tiles than ranks
SHARD_CASES = [(n, tile, frame) for frame in SHARD_FRAMES for tile in SHARD_TILES for n in SHARD_RANKS] + [(3, 16, (96, 64))]
