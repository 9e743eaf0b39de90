"""Reference of art_auto_exposure_device and art_display_device written from the header comment of include/art_hip.h alone: plain numpy
over the pixels, binary32 arrays except where the header names binary64, its own transcription of ART-M1's log_pos, exp_small and apow.
Also the runner of tests/display_host/display_host -- the product's text (csrc/art_display.h) compiled by g++ as a stand-alone program
-- and the frames and cases the tests of the two calls share."""
import itertools
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
U32 = np.uint32
H64 = float.fromhex
QNAN = np.array([0x7fc00000], U32).view(F)[0]
STATE_WORDS = 4 + 256
CURVE_REFERENCE, CURVE_LINEAR, CURVE_REINHARD, CURVE_ACES = 0, 1, 2, 3
TRANSFER_SQRT, TRANSFER_SRGB, TRANSFER_GAMMA22 = 0, 1, 2
LAYOUT_ADA_XY, LAYOUT_ROW_MAJOR = 0, 1
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64)
DEFAULTS = dict(scale=1.0, min_log2=-12.0, max_log2=4.0, low_fraction=0.5, high_fraction=0.95, key=0.18, adapt=1.0, min_exposure=2.0 ** -10,
                max_exposure=2.0 ** 10)

# ---- ART-M1 (csrc/art_math.h): binary64 with + - * / only ---------------------------------------------------------------------------
LOG2E, LN2 = H64("0x1.71547652b82fep+0"), H64("0x1.62e42fefa39efp-1")
SQRT2 = H64("0x1.6a09e667f3bcdp+0")
LOG_C = [H64(c) for c in ("0x1.8618618618618p-5", "0x1.af286bca1af28p-5", "0x1.e1e1e1e1e1e1ep-5", "0x1.1111111111111p-4", "0x1.3b13b13b13b14p-4",
                          "0x1.745d1745d1746p-4", "0x1.c71c71c71c71cp-4", "0x1.2492492492492p-3", "0x1.999999999999ap-3", "0x1.5555555555555p-2")]
LN2_HI, LN2_LO = H64("0x1.62e42fee00000p-1"), H64("0x1.a39ef35793c76p-33")
EXP_C = [H64(c) for c in ("0x1.6124613a86d09p-33", "0x1.1eed8eff8d898p-29", "0x1.ae64567f544e4p-26", "0x1.27e4fb7789f5cp-22", "0x1.71de3a556c734p-19",
                          "0x1.a01a01a01a01ap-16", "0x1.a01a01a01a01ap-13", "0x1.6c16c16c16c17p-10", "0x1.1111111111111p-7", "0x1.5555555555555p-5",
                          "0x1.5555555555555p-3")] + [0.5, 1.0, 1.0]


def log_pos(x):
    """binary64 array, positive and normal -> ln(x)"""
    x = np.ascontiguousarray(x, np.float64)
    b = x.view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    m = ((b & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)).view(np.float64)
    big = m > SQRT2
    m = np.where(big, m * 0.5, m)
    e = e + big
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    q = np.full_like(x, LOG_C[0])
    for c in LOG_C[1:]:
        q = q * z + c
    lm = 2.0 * s + (2.0 * s) * (z * q)
    return e.astype(np.float64) * LN2 + lm


def exp_small(t):
    """binary64 array, |t| <= 200 -> exp(t)"""
    t = np.asarray(t, np.float64)
    v = t * LOG2E
    k = np.trunc(v + np.where(v >= 0.0, 0.5, -0.5))
    r = (t - k * LN2_HI) - k * LN2_LO
    q = np.full_like(t, EXP_C[0])
    for c in EXP_C[1:]:
        q = q * r + c
    return q * np.ldexp(1.0, k.astype(np.int64))


def apow(x, y):
    """Ada's "**" on binary32 as art_math.h spells it: the special cases in its order, else exp_small(y * log_pos(x)) rounded once"""
    with np.errstate(all="ignore"):
        x, y = np.broadcast_arrays(np.asarray(x, F), np.asarray(y, F))
        x, y = x.copy(), y.copy()
        general = np.isfinite(x) & (x > 0)
        t = np.zeros(x.shape)
        t[general] = y[general].astype(np.float64) * log_pos(x[general].astype(np.float64))
        out = np.zeros(x.shape, F)
        mid = general & (t >= -200.0) & (t <= 200.0)
        out[mid] = exp_small(t[mid]).astype(F)
        out[general & (t > 200.0)] = np.inf
        for mask, value in ((np.isinf(x) & (x > 0), np.where(y > 0, F(np.inf), F(0))), (y == F(0.5), np.sqrt(x)), (y == 2, x * x), (y == 1, x), (x == 1, F(1)),
                            (x == 0, np.where(y < 0, F(np.inf), F(0))), (y == 0, F(1)), (x < 0, QNAN), ((x == 0) & (y == 0), QNAN),
                            (np.isnan(x) | np.isnan(y), QNAN)):      # (the last that applies is the first of the header's order)
            out = np.where(mask, value, out).astype(F)
        return out


def amin(a, b):
    return np.where(a < b, a, b).astype(F)


def amax(a, b):
    return np.where(a >= b, a, b).astype(F)


def aclamp(v, lo, hi):
    return amin(amax(v, lo), hi)


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


# ---- auto-exposure ----------------------------------------------------------------------------------------------------------------
def new_state():
    return np.zeros(STATE_WORDS, U32)


def histogram(color, scale=1.0, min_log2=-12.0, max_log2=4.0, **_):
    with np.errstate(all="ignore"):
        c = np.asarray(color, F).reshape(-1, 3) * F(scale)
        assert c.dtype == F
        l = lum(c)
        counted = np.isfinite(l) & (l > 0)
        lo, hi = float(F(min_log2)), float(F(max_log2))
        L = log_pos(l[counted].astype(np.float64)) * LOG2E
        t = ((L - lo) / (hi - lo)) * 254.0
        k = np.where(t < 0, 0.0, np.where(t >= 253.0, 253.0, np.floor(t))).astype(np.int64)
        hist = np.bincount(1 + k, minlength=256).astype(U32)
        hist[0] = (~counted).sum()
        return hist


def auto_exposure(color, state, **kw):
    """the state [260 uint32] after art_auto_exposure_device on color [H, W, 3]"""
    kw = dict(DEFAULTS, **kw)
    state = np.array(state, U32)
    hist = histogram(color, **kw)
    state[4:] = hist
    frames, prev = int(state[3]), state[0:1].view(F)[0]
    N = float(sum(int(c) for c in hist[1:255]))
    a, b = float(F(kw["low_fraction"])) * N, float(F(kw["high_fraction"])) * N
    lo2, span = float(F(kw["min_log2"])), float(F(kw["max_log2"])) - float(F(kw["min_log2"]))
    W = S = cum = 0.0
    for i in range(1, 255):
        lo, hi = cum, cum + float(hist[i])
        o = (hi if hi < b else b) - (lo if lo > a else a)
        centre = lo2 + ((float(i - 1) + 0.5) / 254.0) * span
        if o > 0.0:
            W += o
            S += o * centre
        cum = hi
    if N == 0 or not W > 0.0:
        state[0:1].view(F)[0] = prev if frames else F(1)
        if not frames:
            state[1] = 0
        state[2] = 0
        return state
    with np.errstate(all="ignore"):
        m = F(S / W)
        target = aclamp(F(kw["key"]) * apow(F(2), -m), F(kw["min_exposure"]), F(kw["max_exposure"]))
        e = F(prev + (target - prev) * F(kw["adapt"])) if frames else F(target)
    assert np.asarray(e).dtype == F and np.asarray(target).dtype == F
    state[0:1].view(F)[0] = e
    state[1:2].view(F)[0] = m
    state[2] = int(N)
    state[3] = min(frames + 1, 0xffffffff)
    return state


def exposure_of(state):
    return np.asarray(state, U32)[0:1].view(F)[0]


# ---- display ----------------------------------------------------------------------------------------------------------------------
def round_u32(s):
    """ada_round_u32"""
    with np.errstate(all="ignore"):
        t = np.trunc(np.where(s > 0, s, F(0))).astype(F)
        q = t.astype(np.int64) + ((s - t) >= F(0.5))
        return np.where(s > 0, q, 0)


def pack(q):
    q = np.minimum(q, 255).astype(U32)
    return q[..., 0] | (q[..., 1] << U32(8)) | (q[..., 2] << U32(16))


def display(color, state=None, exposure=1.0, scale=1.0, curve=CURVE_ACES, transfer=TRANSFER_SRGB, white=4.0, dither=1, layout=LAYOUT_ROW_MAJOR):
    """color [H, W, 3] -> (screen uint32, ldr float32 or None for the reference curve), [H, W, ..] or [W, H, ..] by layout"""
    with np.errstate(all="ignore"):
        color = np.asarray(color, F)
        H, W = color.shape[:2]
        if curve == CURVE_REFERENCE:
            g = apow(color * F(scale), F(0.5))
            screen, ldr = pack(round_u32(amin(g, F(1)) * F(255))), None
        else:
            e = exposure_of(state) if state is not None else F(exposure)
            k = F(scale) * e
            x = color * k
            x = np.where(np.isfinite(x) & (x > 0), x, F(0)).astype(F)
            x = amin(x, F(2.0 ** 60))
            if curve == CURVE_LINEAR:
                v = x
            elif curve == CURVE_REINHARD:
                v = (x * (F(1) + x / (F(white) * F(white)))) / (F(1) + x)
            else:
                v = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
            v = aclamp(v, F(0), F(1))
            if transfer == TRANSFER_SQRT:
                u = np.sqrt(v)
            elif transfer == TRANSFER_SRGB:
                u = np.where(v < F(0.0031308), F(12.92) * v, F(1.055) * apow(v, F(H64("0x1.aaaaaap-2"))) - F(0.055))
            else:
                u = apow(v, F(H64("0x1.d1745ep-2")))
            assert u.dtype == F and v.dtype == F
            s = u * F(255)
            if dither:
                Y, X = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
                d = (BAYER[Y & 3, X & 3].astype(F) + F(0.5)) / F(16)
                q = np.trunc(s + d[..., None]).astype(np.int64)
            else:
                q = round_u32(s)
            screen, ldr = pack(q), u
        if layout == LAYOUT_ADA_XY:
            screen = np.ascontiguousarray(screen.T)
            ldr = None if ldr is None else np.ascontiguousarray(ldr.transpose(1, 0, 2))
        return screen, ldr


def differ(a, b):
    """number of 32-bit words that differ"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == 4 and b.dtype.itemsize == 4, (a.shape, b.shape)
    return int((a.view(U32) != b.view(U32)).sum())


# ---- the g++ build of the product's text ------------------------------------------------------------------------------------------
_built = False


def host_program():
    global _built
    d = os.path.join(HERE, "display_host")
    if not _built:
        subprocess.check_call(["make", "-s", "-C", d, "display_host"])
        _built = True
    return os.path.join(d, "display_host")


def auto_exposure_host(color, state, **kw):
    """auto_exposure() through csrc/art_display.h compiled by g++ (a stand-alone program: IN and OUT are files)"""
    kw = dict(DEFAULTS, **kw)
    color = np.ascontiguousarray(color, F)
    H, W = color.shape[:2]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<2i9f", W, H, *[kw[n] for n in ("scale", "min_log2", "max_log2", "low_fraction", "high_fraction", "key", "adapt",
                                                                    "min_exposure", "max_exposure")]))
            f.write(np.ascontiguousarray(state, U32).tobytes()); f.write(color.tobytes())
        subprocess.check_call([host_program(), "exposure", fin, fout])
        return np.fromfile(fout, U32)


def display_host(color, state=None, exposure=1.0, scale=1.0, curve=CURVE_ACES, transfer=TRANSFER_SRGB, white=4.0, dither=1, layout=LAYOUT_ROW_MAJOR,
                 want_screen=True, want_ldr=True):
    """display() through the same program; ldr is None where it is not wanted (the reference curve has none)"""
    color = np.ascontiguousarray(color, F)
    H, W = color.shape[:2]
    want_ldr = want_ldr and curve != CURVE_REFERENCE
    shape = (H, W) if layout == LAYOUT_ROW_MAJOR else (W, H)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<2i2f2if2i", W, H, scale, exposure, curve, transfer, white, int(dither), layout))
            f.write(struct.pack("<2i", state is not None, (1 if want_screen else 0) | (2 if want_ldr else 0)))
            f.write(np.ascontiguousarray(state if state is not None else new_state(), U32).tobytes()); f.write(color.tobytes())
        subprocess.check_call([host_program(), "display", fin, fout])
        words = np.fromfile(fout, U32)
    n = W * H
    screen = words[:n].reshape(shape) if want_screen else None
    ldr = words[n if want_screen else 0:].view(F).reshape(shape + (3,)) if want_ldr else None
    return screen, ldr


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (37, 23), (67, 131)]       # (W, H): one pixel; odd and not square; more than one workgroup's stride of 256, width no multiple of 64
CURVES = (CURVE_REFERENCE, CURVE_LINEAR, CURVE_REINHARD, CURVE_ACES)
TRANSFERS = (TRANSFER_SQRT, TRANSFER_SRGB, TRANSFER_GAMMA22)


def layouts(W, H):
    return (LAYOUT_ROW_MAJOR,) if W == H else (LAYOUT_ROW_MAJOR, LAYOUT_ADA_XY)


def hdr_frame(W, H, seed=0, lo=1e-3, hi=50.0):
    """a frame of colours log-uniform in [lo, hi] per channel: every luminance inside the default range of the histogram"""
    rng = np.random.default_rng(104729 * W + 257 * H + seed)
    return np.exp(rng.uniform(np.log(lo), np.log(hi), (H, W, 3))).astype(F)


def green_of_luminance(l):
    """a green value g with 0.7152f * g == l in binary32 (the colour (0, g, 0) then has exactly that luminance)"""
    l = F(l)
    g = F(l / F(0.7152))
    for _ in range(8):
        g = np.nextafter(g, F(0))
    for _ in range(17):
        if F(0.7152) * g == l:
            return g
        g = np.nextafter(g, F(np.inf))
    raise AssertionError("no green gives the luminance %r" % l)


def spots(H, W, k):
    """k-th of a few pixel positions spread over the frame"""
    return ((k * 5 + 1) % H, (k * 7 + 2) % W)


def special_frame(W, H, seed=0):
    """an HDR frame with the pixels the header's rules are about planted over it (as many as the frame has room for): channels that are
    NaN, infinite, negative, zero, denormal or huge, highlights far above 1, and luminances exactly on, just under and just over bin
    edges of the range -12 .. 4 (the edge between bins i and i + 1 is at log2 = -12 + 16 i / 254: an integer for i = 127) and outside it"""
    c = hdr_frame(W, H, seed)
    edge = [green_of_luminance(2.0 ** -4), np.nextafter(green_of_luminance(2.0 ** -4), F(0)), np.nextafter(green_of_luminance(2.0 ** -4), F(1)),
            green_of_luminance(2.0 ** -12), np.nextafter(green_of_luminance(2.0 ** -12), F(0)), green_of_luminance(2.0 ** 4),
            np.nextafter(green_of_luminance(2.0 ** 4), F(0))]
    px = [(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (-1, 2, 3), (-5, -5, -5), (0, 0, 0), (-0.0, 0.0, -0.0), (1e-40, 1e-40, 1e-40), (0, 1e-45, 0),
          (3e38, 3e38, 3e38), (1e30, 0, 0), (1e-6, 1e-6, 1e-6), (100, 100, 100), (1000, 0.5, 0.01), (np.nan, np.nan, np.nan), (np.inf, np.inf, np.inf),
          (1, 1, 1), (0.18, 0.18, 0.18), (0.0031308, 0.0031307, 0.0031309), (2e19, 2e19, 2e19)] + [(0, g, 0) for g in edge]
    flat = c.reshape(-1, 3)
    for k, p in enumerate(px):
        if k < W * H - 1 or (W * H == 1 and k == 0):
            y, x = spots(H, W, k)
            flat[(y * W + x + k) % (W * H)] = np.array(p, F)
    return c


def exposure_cases(W, H):
    """(name, [frames of one sequence on one state], keyword arguments of auto_exposure())"""
    black = np.zeros((H, W, 3), F)
    one_bin = np.broadcast_to(np.array([0.25, 0.3, 0.2], F), (H, W, 3)).copy()
    seq = [hdr_frame(W, H, 1), hdr_frame(W, H, 2, 0.05, 400.0), hdr_frame(W, H, 3, 1e-3, 2.0)]
    return [("defaults", seq, {}),
            ("adapt_quarter", seq, dict(adapt=0.25)),
            ("specials", [special_frame(W, H), special_frame(W, H, 5)], dict(adapt=0.5)),
            ("scaled", [hdr_frame(W, H, 4) * F(16)], dict(scale=1.0 / 16)),
            ("black_fresh_then_valid", [black, seq[0], seq[1]], dict(adapt=0.25)),
            ("black_after_valid", [seq[0], black, np.full((H, W, 3), -1.0, F), seq[1]], dict(adapt=0.5)),
            ("one_bin", [one_bin, one_bin], dict(adapt=0.5)),
            ("one_bin_trim_inside_it", [one_bin], dict(low_fraction=0.3, high_fraction=0.7)),
            ("no_trimming", seq[:2], dict(low_fraction=0.0, high_fraction=1.0)),
            ("range_ends_inside_a_bin", [seq[0]], dict(low_fraction=0.123, high_fraction=0.777)),
            ("narrow_range_everything_outside", [seq[1]], dict(min_log2=-1.0, max_log2=-0.5, low_fraction=0.0, high_fraction=1.0)),
            ("denormal_luminances", [hdr_frame(W, H, 6) * F(1e-41)], dict(min_log2=-126.0, max_log2=-100.0)),
            ("clamped_to_the_bounds", [seq[0], seq[0] * F(1e-6)], dict(min_exposure=0.5, max_exposure=2.0))]


def display_cases(W, H):
    """(name, keyword arguments of display()) at one frame size: every curve x transfer x dither in every layout over the special frame"""
    c = special_frame(W, H, 2)
    st = new_state()
    st[0:1].view(F)[0] = F(0.37)
    out = []
    for curve, transfer, dither, layout in itertools.product(CURVES, TRANSFERS, (0, 1), layouts(W, H)):
        out.append(("curve%d_transfer%d_dither%d_layout%d" % (curve, transfer, dither, layout),
                    dict(color=c, exposure=1.7, scale=0.25, curve=curve, transfer=transfer, white=3.0, dither=dither, layout=layout)))
    out.append(("exposure_from_state", dict(color=c, state=st, exposure=123.0, scale=1.0, curve=CURVE_ACES, transfer=TRANSFER_SRGB, dither=1)))
    bad = new_state()
    bad[0] = 0x7fc00000
    out.append(("exposure_nan_in_state", dict(color=c, state=bad, curve=CURVE_REINHARD, transfer=TRANSFER_GAMMA22, dither=0)))
    out.append(("exposure_zero", dict(color=c, exposure=0.0, curve=CURVE_LINEAR, transfer=TRANSFER_SRGB, dither=1)))
    ramp = (np.arange(W * H * 3, dtype=np.float64).reshape(H, W, 3) / max(1, W * H * 3 - 1)).astype(F)
    out.append(("ramp_linear_srgb", dict(color=ramp, curve=CURVE_LINEAR, transfer=TRANSFER_SRGB, dither=0)))
    out.append(("ramp_reference", dict(color=ramp * F(4), scale=0.25, curve=CURVE_REFERENCE)))
    return out
