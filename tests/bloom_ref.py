"""Reference of art_bloom_device written from the header comment of include/art_hip.h alone: plain numpy over whole levels, binary32
arrays, every operation one numpy operation (so each is rounded once, in the header's order).  Also the runner of
tests/bloom_host/bloom_host -- the product's per-texel text (csrc/art_bloom.h) compiled by g++ as a stand-alone program -- and the
synthetic frames and cases the tests of the call share."""
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
U32 = np.uint32
TAIL_TEXELS = 4096      # bl::kTailTexels (csrc/art_bloom.h): what one workgroup holds


def lum3(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def amax(a, b):
    return np.where(a >= b, a, b).astype(F)


def amin(a, b):
    return np.where(a < b, a, b).astype(F)


def sanitise(color, scale):
    """the read rule: s(p)"""
    s = (F(scale) * np.asarray(color, F)).astype(F)
    s = np.where(np.isfinite(s) & (s > 0), s, F(0)).astype(F)
    return amin(s, F(2.0 ** 60))


def prefilter(s, e, threshold, knee):
    threshold, knee, e = F(threshold), F(knee), F(e)
    if threshold == 0 and knee == 0:
        return s
    l = (e * lum3(s)).astype(F)
    ok = np.isfinite(l) & (l > 0)
    q = amin(amax((l - (threshold - knee)).astype(F), F(0)), F(2) * knee)
    soft = ((q * q).astype(F) / (F(4) * knee)).astype(F) if knee > 0 else np.zeros_like(l)
    c = amax(soft, amax((l - threshold).astype(F), F(0)))
    f = np.where(ok, amin((c / np.where(ok, l, F(1))).astype(F), F(1)), F(0)).astype(F)
    return (f[..., None] * s).astype(F)


def level_sizes(W, H, levels):
    """[(w_0, h_0), (w_1, h_1), .. (w_M, h_M)]"""
    out = [(W, H)]
    for _ in range(levels):
        w, h = out[-1]
        out.append(((w + 1) >> 1, (h + 1) >> 1))
        if out[-1] == (1, 1):
            break
    return out


def down(A, karis=False):
    """level k + 1 from level k ([h, w, 3])"""
    h, w = A.shape[:2]
    hd, wd = (h + 1) >> 1, (w + 1) >> 1
    rows = [np.clip(2 * np.arange(hd) - 2 + i, 0, h - 1) for i in range(6)]
    cols = [np.clip(2 * np.arange(wd) - 2 + j, 0, w - 1) for j in range(6)]
    t = [[A[rows[i]][:, cols[j]] for j in range(6)] for i in range(6)]

    def Q(a, b):
        return (((t[b][a] + t[b][a + 1]) + (t[b + 1][a] + t[b + 1][a + 1])) * F(0.25)).astype(F)
    inner = (Q(1, 1) + Q(3, 1)) + (Q(1, 3) + Q(3, 3))
    if not karis:
        edge = (Q(2, 0) + Q(0, 2)) + (Q(4, 2) + Q(2, 4))
        corner = (Q(0, 0) + Q(4, 0)) + (Q(0, 4) + Q(4, 4))
        return ((F(0.125) * (inner + Q(2, 2)) + F(0.0625) * edge) + F(0.03125) * corner).astype(F)
    g = [inner * F(0.25), ((Q(0, 0) + Q(2, 0)) + (Q(0, 2) + Q(2, 2))) * F(0.25), ((Q(2, 0) + Q(4, 0)) + (Q(2, 2) + Q(4, 2))) * F(0.25),
         ((Q(0, 2) + Q(2, 2)) + (Q(0, 4) + Q(2, 4))) * F(0.25), ((Q(2, 2) + Q(4, 2)) + (Q(2, 4) + Q(4, 4))) * F(0.25)]
    k = [(F(0.5 if n == 0 else 0.125) / (F(1) + lum3(g[n]))).astype(F)[..., None] for n in range(5)]
    K = ((k[1] + k[2]) + (k[3] + k[4])) + k[0]
    return (((((k[1] * g[1]) + (k[2] * g[2])) + ((k[3] * g[3]) + (k[4] * g[4]))) + (k[0] * g[0])) / K).astype(F)


def up(S, wd, hd):
    """up(S, ws, hs) at every (x, y) of a wd x hd level"""
    hs, ws = S.shape[:2]
    x, y = np.arange(wd), np.arange(hd)
    xn, yn = x >> 1, y >> 1
    xf = np.clip(np.where(x & 1, xn + 1, xn - 1), 0, ws - 1)
    yf = np.clip(np.where(y & 1, yn + 1, yn - 1), 0, hs - 1)
    top = F(0.75) * S[yn][:, xn] + F(0.25) * S[yn][:, xf]
    bot = F(0.75) * S[yf][:, xn] + F(0.25) * S[yf][:, xf]
    return (F(0.75) * top + F(0.25) * bot).astype(F)


def bloom(color, levels=6, karis=1, scale=1.0, exposure=1.0, threshold=0.0, knee=0.0, scatter=0.7, strength=0.05, state_exposure=None, variant=0):
    """color [H, W, 3] -> (out, bloom, D, U): the two outputs and the levels 1 .. M after the down sweep and after the up sweep.
    state_exposure: word 0 of the exposure state, or None = `exposure`.  variant changes no word and is not read."""
    with np.errstate(all="ignore"):
        color = np.asarray(color, F)
        H, W = color.shape[:2]
        s = sanitise(color, scale)
        sizes = level_sizes(W, H, levels)
        M = len(sizes) - 1
        D = [prefilter(s, exposure if state_exposure is None else state_exposure, threshold, knee)]
        for k in range(M):
            D.append(down(D[k], karis=bool(karis) and k == 0))
            assert D[-1].shape[:2] == sizes[k + 1][::-1]
        U = [None] * (M + 1)
        U[M] = D[M]
        for k in range(M - 1, 0, -1):
            U[k] = (D[k] + F(scatter) * (up(U[k + 1], *sizes[k]) - D[k])).astype(F)
        B = up(U[1], W, H)
        out = (s + F(strength) * (B - s)).astype(F)
        return out, B, D[1:], U[1:]


def differ(a, b):
    """number of words that differ, bit for bit"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(U32) != b.view(U32)).sum())


def differ_all(got, want):
    """over (out, bloom, D, U) of bloom() and bloom_host(), or (out, bloom) pairs"""
    n = differ(got[0], want[0]) + differ(got[1], want[1])
    for a, b in zip(got[2:], want[2:]):
        assert len(a) == len(b)
        n += sum(differ(x, y) for x, y in zip(a, b))
    return n


def tail_first(W, H, levels, variant=0):
    """the first level of the tail (the header of csrc/art_bloom.h states the rule), or 0"""
    n = [w * h for w, h in level_sizes(W, H, levels)]
    M = len(n) - 1
    if variant == 0:
        for k in range(1, M):
            if sum(n[k:]) <= TAIL_TEXELS:
                return k
    return 0


def launches(W, H, levels, variant):
    """the kernel launches of one call"""
    M = len(level_sizes(W, H, levels)) - 1
    T = tail_first(W, H, levels, variant)
    return 2 * T + 1 if T else 2 * M


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
_built = False


def host_program():
    global _built
    d = os.path.join(HERE, "bloom_host")
    if not _built:
        subprocess.check_call(["make", "-s", "-C", d, "bloom_host"])
        _built = True
    return os.path.join(d, "bloom_host")


def bloom_host(color, levels=6, karis=1, scale=1.0, exposure=1.0, threshold=0.0, knee=0.0, scatter=0.7, strength=0.05, state_exposure=None, variant=0,
               in_place=False):
    """the same call through csrc/art_bloom.h compiled by g++ (a stand-alone program: IN and OUT are files); in_place: out3f is color3f"""
    color = np.ascontiguousarray(color, F)
    H, W = color.shape[:2]
    given = (1 if state_exposure is not None else 0) | (2 if in_place else 0)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<5i6fif", W, H, levels, karis, variant, scale, exposure, threshold, knee, scatter, strength, given,
                                0.0 if state_exposure is None else state_exposure))
            f.write(color.tobytes())
        subprocess.check_call([host_program(), "run", fin, fout])
        raw = np.fromfile(fout, F)
    n = 3 * W * H
    out, B = raw[:n].reshape(H, W, 3), raw[n:2 * n].reshape(H, W, 3)
    sizes = level_sizes(W, H, levels)[1:]
    at, sweeps = 2 * n, []
    for _ in range(2):
        lv = []
        for w, h in sizes:
            rec = raw[at:at + 4 * w * h].reshape(h, w, 4)
            assert not rec[..., 3].view(U32).any()          # a record's fourth word is +0
            lv.append(rec[..., :3])
            at += 4 * w * h
        sweeps.append(lv)
    assert at == raw.size
    return out, B, sweeps[0], sweeps[1]


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
# (W, H): one pixel; one tile and less; odd sizes; a level wider than a tile (130 x 4: level 1 is 65 x 2); 70 x 66 and 130 x 70: the tail
# starts at level 1; 300 x 120: one level (150 x 60) has launches of its own before the tail
SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (33, 31), (130, 4), (70, 66), (130, 70), (300, 120)]
LEVELS = (1, 2, 8)


def frame(W, H, seed=0):
    """an HDR frame as an accum of 4 colours: a smooth ramp with noise, and a few lights 100 to 3000 times their surroundings, one of
    them in a corner and one on an edge"""
    rng = np.random.default_rng(7919 * W + 389 * H + seed)
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    base = (0.3 + 0.03 * X + 0.02 * Y)[..., None] * np.array([1.0, 0.8, 0.6]) * rng.uniform(0.5, 1.5, (H, W, 3))
    for k in range(max(2, (W * H) // 300)):
        y, x = ((k * 13) % H, (k * 29) % W) if k else (0, 0)
        base[y, x] *= 100.0 * (1 + 3 * (k % 10))
    base[H - 1, W // 2] *= 500.0
    return (4.0 * base).astype(F)


def planted_bad(color):
    """NaN, +-inf, negative and > 2^60 channels at the frame's corners, at tile corners, in halos and at spread positions"""
    H, W = color.shape[:2]
    color = color.copy()
    bads = (np.nan, np.inf, -np.inf, -3.0, 3e38, 5e18, -0.0)
    places = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (15, 15), (16, 16), (31, 32), (33, 3), (3, 33), (16, 0), (0, 16)]
    places += [((k * 5 + 1) % H, (k * 7 + 2) % W) for k in range(8)]
    for k, (y, x) in enumerate(places):
        if y < H and x < W:
            color[y, x, k % 3] = bads[k % len(bads)]
    color.view(U32)[(H // 2), (W // 2), 1] = 0xffc12345
    return color


def cases(W, H):
    """(name, keyword arguments of bloom()) at one frame size"""
    c = frame(W, H)
    bad = planted_bad(c)
    out = []
    for levels in LEVELS:
        out.append(("levels %d, karis" % levels, dict(color=c, levels=levels, karis=1, scale=0.25, scatter=0.7, strength=0.05)))
        out.append(("levels %d, no karis" % levels, dict(color=c, levels=levels, karis=0, scale=0.25, scatter=0.5, strength=0.25)))
        out.append(("levels %d, per level" % levels, dict(color=c, levels=levels, karis=1, scale=0.25, scatter=0.7, strength=0.05, variant=1)))
    out.append(("threshold alone", dict(color=c, levels=8, karis=1, scale=0.25, threshold=1.0, knee=0.0, exposure=0.5)))
    out.append(("threshold and knee", dict(color=c, levels=8, karis=0, scale=0.25, threshold=1.0, knee=0.5, exposure=0.5, scatter=0.3, strength=1.0)))
    out.append(("knee above the threshold, a state", dict(color=c, levels=3, karis=1, scale=0.25, threshold=0.25, knee=1.0, exposure=7.0, state_exposure=0.125)))
    out.append(("a state without a threshold", dict(color=c, levels=2, karis=1, scale=0.25, state_exposure=float("nan"))))
    out.append(("a state that is not finite", dict(color=c, levels=2, karis=0, scale=0.25, threshold=0.5, knee=0.25, state_exposure=float("inf"))))
    out.append(("exposure 0", dict(color=c, levels=2, karis=0, scale=0.25, threshold=0.5, knee=0.25, exposure=0.0, strength=0.5)))
    out.append(("a huge knee", dict(color=c, levels=2, karis=0, scale=0.25, threshold=1.0, knee=3e38, exposure=1.0, strength=0.5)))
    for sc, st in ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)):
        out.append(("scatter %g strength %g" % (sc, st), dict(color=c, levels=8, karis=1, scale=0.25, scatter=sc, strength=st)))
    out.append(("planted bad", dict(color=bad, levels=8, karis=1, scale=0.25)))
    out.append(("planted bad, threshold, per level", dict(color=bad, levels=8, karis=0, scale=1.0, threshold=2.0, knee=1.0, exposure=0.25, strength=0.5, variant=1)))
    out.append(("planted bad, a huge scale", dict(color=bad, levels=3, karis=1, scale=1e30, threshold=0.0, knee=0.5, exposure=1e-30, strength=0.5)))
    out.append(("a negative scale", dict(color=c, levels=2, karis=1, scale=-1.0, strength=1.0)))
    out.append(("black", dict(color=np.zeros((H, W, 3), F), levels=8, karis=1, scale=1.0, threshold=0.5, knee=0.5, strength=0.5)))
    return out
