"""Reference of the luminance moments of art_bind_moments, written from the header comment of include/art_hip.h: the per-sample radiance
comes from the CPU oracle (orc_sample_radiance through orc.lib(), with this file's own declaration of its arguments), the colours, their
luminance and the running sums are numpy binary32 over the pixels, with Python loops over the samples, in the order the header states."""
import concurrent.futures
import ctypes as C

import numpy as np

import orc

F = np.float32


def _sample_fn():
    fn = orc.lib().orc_sample_radiance
    fn.argtypes = [C.POINTER(orc.Scene), C.POINTER(orc.Params), C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_float)]
    fn.restype = None
    return fn


def sample_radiance(scene, prm, first, count, workers=8):
    """radiance of the camera samples first .. first + count - 1 of every pixel of the frame prm describes: [count, H, W, 3] float32.
    (The oracle call releases the interpreter lock, so the rows are shared among a few threads; every word has one writer.)"""
    fn = _sample_fn()
    W, H = prm.width, prm.height
    out = np.zeros((count, H, W, 3), F)
    ps, pp = C.byref(scene), C.byref(prm)

    def rows(y0, y1):
        for y in range(y0, y1):
            for x in range(W):
                for s in range(count):
                    fn(ps, pp, x, y, first + s, out[s, y, x].ctypes.data_as(C.POINTER(C.c_float)))
    step = max(1, (H + workers - 1) // workers)
    with concurrent.futures.ThreadPoolExecutor(workers) as ex:
        for f in [ex.submit(rows, y0, min(H, y0 + step)) for y0 in range(0, H, step)]:
            f.result()
    return out


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def colours(rad, aa_on, background=(0.0, 0.0, 0.0)):
    """rad [S, ..., 3] in sample order -> the colours a pass adds to the accum, in order: with aa_on (((bg + s0) + s1) + s2) + s3 per group
    of four samples, else every sample"""
    rad = np.asarray(rad, F)
    if not aa_on:
        return rad
    assert rad.shape[0] % 4 == 0
    out = np.zeros((rad.shape[0] // 4,) + rad.shape[1:], F)
    for k in range(out.shape[0]):
        c = np.broadcast_to(np.asarray(background, F), rad.shape[1:]).astype(F)
        for i in range(4):
            c = c + rad[4 * k + i]
        out[k] = c
    return out


def add_colours(cols, accum=None, moments=None):
    """the running sums after the colours cols [n, ..., 3], from accum [..., 3] and moments [..., 2] (zeros when None):
    accum = colour + accum;  l = lum(colour);  S1 = l + S1;  S2 = l * l + S2, all binary32"""
    with np.errstate(all="ignore"):
        cols = np.asarray(cols, F)
        a = np.zeros(cols.shape[1:], F) if accum is None else np.array(accum, F, copy=True)
        m = np.zeros(cols.shape[1:-1] + (2,), F) if moments is None else np.array(moments, F, copy=True)
        for c in cols:
            a = c + a
            l = lum(c)
            m[..., 0] = l + m[..., 0]
            m[..., 1] = l * l + m[..., 1]
        assert a.dtype == F and m.dtype == F
        return a, m
