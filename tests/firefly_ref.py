"""Reference of art_firefly_device written from the header comment of include/art_hip.h alone: plain numpy over the pixels, binary32
arrays, a Python loop over the offsets of the window and a sort for the rank.  Also the runner of tests/firefly_host/firefly_host -- the
product's per-pixel text (csrc/art_firefly.h) compiled by g++ as a stand-alone program -- and the synthetic frames and cases the tests of
the call share."""
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
U32 = np.uint32
QNAN = np.array([0x7fc00000], U32).view(F)[0]


def lum3(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def quiet(a):
    a = np.array(a, F)
    a.view(U32)[np.isnan(a)] = 0x7fc00000
    return a


def firefly(color, moments=None, ids=None, radius=1, rank=1, min_count=None, scale=1.0, gain=2.0, floor=0.0):
    """color [H, W, 3], moments [H, W, 2] or None, ids [H, W] int32 or None -> (out [H, W, 3], moments_out or None, clamped [H, W] uint8).
    The inputs are not written: 'in place' in this reference's terms is the caller handing the results back as the next inputs."""
    with np.errstate(all="ignore"):
        color = np.asarray(color, F)
        H, W = color.shape[:2]
        min_count = rank if min_count is None else min_count
        scale, gain, floor = F(scale), F(gain), F(floor) + F(0)
        c = (scale * color).astype(F)
        l = lum3(c).astype(F)
        bad = ~(np.isfinite(c).all(-1) & np.isfinite(l))
        key = np.where(bad, QNAN, l).astype(F)
        # the neighbours' keys, one layer per offset; what is no neighbour is -infinity and is not counted
        layers = []
        ys, xs = np.mgrid[0:H, 0:W]
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if dx == 0 and dy == 0:
                    continue
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                is_n = inside & ~bad[qy, qx]
                if ids is not None:
                    is_n &= ids[qy, qx] == ids
                layers.append(np.where(is_n, key[qy, qx], F(-np.inf)).astype(F))
        layers = np.stack(layers, 0)
        count = (layers != F(-np.inf)).sum(0)              # (a key is finite: -infinity is only the filler)
        m = np.sort(layers, axis=0)[::-1][rank - 1]
        T = (gain * m).astype(F) + floor
        T = np.where(T >= F(0), T, F(0)).astype(F)
        clamp = ~bad & (count >= min_count) & (l > T)
        f = (T / l).astype(F)
        out = np.where(clamp[..., None], (f[..., None] * c).astype(F), c).astype(F)
        out = quiet(out)
        mo = None
        if moments is not None:
            moments = np.asarray(moments, F).reshape(-1)[:2 * H * W].reshape(H, W, 2)
            scaled = quiet(np.stack([(f * moments[..., 0]).astype(F), ((f * f).astype(F) * moments[..., 1]).astype(F)], -1))
            mo = np.where(clamp[..., None], scaled.view(U32), moments.view(U32)).astype(U32).view(F)      # (not clamped: the words as they are)
        flag = np.where(bad, 2, np.where(clamp, 1, 0)).astype(np.uint8)
        return out, mo, flag


def differ(a, b):
    """number of words (bytes of a flag plane) that differ, bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == F:
        a, b = a.view(U32), b.view(U32)
    return int((a != b).sum())


def differ_all(got, want):
    """over (out, moments_out, clamped) triples"""
    assert (got[1] is None) == (want[1] is None)
    return sum(differ(a, b) for a, b in zip(got, want) if a is not None)


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
_built = False


def host_program():
    global _built
    d = os.path.join(HERE, "firefly_host")
    if not _built:
        subprocess.check_call(["make", "-s", "-C", d, "firefly_host"])
        _built = True
    return os.path.join(d, "firefly_host")


def firefly_host(color, moments=None, ids=None, radius=1, rank=1, min_count=None, scale=1.0, gain=2.0, floor=0.0, in_place=False):
    """the same call through csrc/art_firefly.h compiled by g++ (a stand-alone program: IN and OUT are files); in_place: out3f is color3f
    and moments_out2f is moments2f"""
    color = np.ascontiguousarray(color, F)
    H, W = color.shape[:2]
    min_count = rank if min_count is None else min_count
    given = (1 if moments is not None else 0) | (2 if ids is not None else 0) | (4 if in_place else 0)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<5i3fi", W, H, radius, rank, min_count, scale, gain, floor, given))
            f.write(color.tobytes())
            if moments is not None:
                f.write(np.ascontiguousarray(moments, F).reshape(-1)[:2 * H * W].tobytes())
            if ids is not None:
                f.write(np.ascontiguousarray(ids, np.int32).tobytes())
        subprocess.check_call([host_program(), "run", fin, fout])
        raw = np.fromfile(fout, np.uint8)
    n = W * H
    out = raw[:12 * n].view(F).reshape(H, W, 3)
    o = 12 * n
    mo = None
    if moments is not None:
        mo = raw[o:o + 8 * n].view(F).reshape(H, W, 2)
        o += 8 * n
    assert raw.size == o + n
    return out, mo, raw[o:].reshape(H, W)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (7, 1), (16, 16), (17, 16), (33, 19), (70, 66)]      # (W, H): one pixel, a window wider than the frame, tile edges with and without a remainder
RADII = (1, 2)


def frame(W, H, seed=0, spikes=True):
    """a noisy frame: luminance around a smooth ramp with a relative noise of a quarter, an id plane of vertical bands and a diagonal,
    moments of 4 colours per pixel whose mean is the colour; with spikes a few pixels 50 to 500 times their surroundings, two of them
    side by side (what rank 2 is for).  Returns (color [H, W, 3] as an accum of 4 colours, moments [H, W, 2], ids [H, W])."""
    rng = np.random.default_rng(104729 * W + 613 * H + seed)
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    base = 0.2 + 0.02 * X + 0.01 * Y
    tint = np.array([1.0, 0.8, 0.6])
    samples = base[..., None, None] * tint * rng.uniform(0.5, 1.5, (H, W, 4, 1)) * rng.uniform(0.9, 1.1, (H, W, 4, 3))
    if spikes:
        for k in range(max(1, (W * H) // 40)):
            y, x = (k * 11 + 3) % H, (k * 17 + 5) % W
            samples[y, x, k % 4] *= 50.0 * (1 + k % 10)
            if k % 3 == 0 and x + 1 < W:
                samples[y, x + 1, 0] *= 120.0
    color = samples.sum(2).astype(F)
    ls = lum3(samples.astype(F)).astype(np.float64)
    moments = np.stack([ls.sum(-1), (ls * ls).sum(-1)], -1).astype(F)
    ids = (((X // 5) % 3) + 10 * (X == Y)).astype(np.int32)
    return color, moments, ids


def spots(H, W, k):
    return ((k * 5 + 1) % H, (k * 7 + 2) % W)


def planted_bad(color, moments):
    """NaN, +-inf and negative channels at a tile corner (15, 15), (16, 16), in a halo (row / column 17), at the frame's corners and at a
    few spread positions; a NaN and an infinity in the moments of pixels that are clamped or not"""
    H, W = color.shape[:2]
    color, moments = color.copy(), moments.copy()
    bads = (np.nan, np.inf, -np.inf, -3.0, -1e30, 3e38)
    places = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (15, 15), (16, 16), (15, 16), (17, 3), (3, 17), (16, 0), (0, 16)]
    places += [spots(H, W, k) for k in range(6)]
    for k, (y, x) in enumerate(places):
        if y < H and x < W:
            color[y, x, k % 3] = bads[k % len(bads)]
    for k in range(4):
        y, x = spots(H, W, 7 + k)
        moments[y, x, k % 2] = (np.nan, np.inf)[k // 2]
    y, x = spots(H, W, 11)
    color.view(U32)[y, x, 1] = 0xffc12345          # a NaN with a sign and a payload: it must leave as the quiet NaN
    return color, moments


def cases(W, H):
    """(name, keyword arguments of firefly()) at one frame size: every parameter at both ends"""
    out = []
    color, moments, ids = frame(W, H)
    bc, bm = planted_bad(color, moments)
    full = {1: 8, 2: 24}
    for radius in RADII:
        for rank in (1, 2, 3, 4):
            out.append(("r%d rank %d" % (radius, rank), dict(color=color, moments=moments, ids=ids if rank % 2 else None, radius=radius, rank=rank, gain=1.0 + rank % 2 * 3.0,
                                                             floor=0.0 if rank < 3 else 0.05, scale=0.25)))
        out.append(("r%d min_count full" % radius, dict(color=color, moments=moments, radius=radius, rank=2, min_count=full[radius], gain=1.0, scale=0.25)))
        out.append(("r%d min_count full, ids" % radius, dict(color=color, moments=None, ids=ids, radius=radius, rank=1, min_count=full[radius], gain=4.0, scale=1.0)))
        out.append(("r%d no moments, scale 1" % radius, dict(color=color, radius=radius, rank=1, gain=4.0, floor=0.5, scale=1.0)))
        out.append(("r%d planted bad" % radius, dict(color=bc, moments=bm, ids=ids, radius=radius, rank=1, gain=1.0, scale=0.25)))
        out.append(("r%d planted bad, rank 3" % radius, dict(color=bc, moments=bm, radius=radius, rank=3, gain=4.0, floor=0.01, scale=1.0)))
        flat = np.full((H, W, 3), 0.375, F)
        out.append(("r%d equal keys" % radius, dict(color=flat, moments=moments, radius=radius, rank=1, gain=1.0, scale=1.0)))
        out.append(("r%d black, floor 0" % radius, dict(color=np.zeros((H, W, 3), F), moments=np.zeros((H, W, 2), F), radius=radius, rank=1, gain=1.0, scale=1.0)))
        neg = color.copy(); neg[::2, ::3] *= F(-1); neg[1::4, 1::2] = F(0); neg[1::4, 1::2, 1] = F(-0.0)
        out.append(("r%d negative and zero keys, floor -0" % radius, dict(color=neg, moments=moments, radius=radius, rank=2, gain=1.0, floor=-0.0, scale=0.25)))
        # gain * m overflows: to +infinity in the right half (nothing is above it), to -infinity in the left half, where every third
        # pixel is positive among negative neighbours: T = 0 and the pixel goes to 0
        huge = color * F(1e30)
        huge[:, :W // 2] *= F(-1); huge[1::3, 1:W // 2:3] *= F(-1)
        out.append(("r%d huge gain" % radius, dict(color=huge, moments=moments, radius=radius, rank=1, gain=3e38, floor=0.0, scale=1.0)))
    return out
