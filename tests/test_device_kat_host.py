"""CPU leg of the per-function known-answer harness (tests/device_kat/kat_ops.h, tests/kat_inputs.py):
  * hs_kat_run -- the ops compiled by g++ -- equals the independent Ada transcription on the edge lists and the first random items, so that a
    failure of tests/test_gpu_device_kat.py on the GPU can be told apart from a failure of the text;
  * the PRODUCT's ART-M1 (csrc/art_math.h: asincos_m1, atan_m1, apow, m1::log_pos, m1::exp_small) is held to mpmath at 120 bits on every
    item of the math sets: correctly rounded binary32 results, binary64 internals below 2^-50 relative error.
Measured on the sets of tests/kat_inputs.py (printed by the tests, -s): sin / cos / tan / apow: 0 results that are not the correctly
rounded value; log_pos: max relative error 2^-51.99 on 100 022 items; exp_small: 2^-52.43 on 120 050 items."""
import numpy as np
import pytest
from mpmath import libmp

import devkat
import kat_inputs as ki
import kat_refs

PREC = 120
RND = "n"
TRANSCRIBED = [op for op in devkat.OPS if not (op in kat_refs.NO_TRANSCRIPTION and kat_refs.NO_TRANSCRIPTION[op] is not None)]


@pytest.mark.parametrize("op", TRANSCRIBED)
def test_host_build_equals_the_transcription(art, op):
    run = kat_refs.host_runner(art, op)
    n = kat_refs.assert_matches_transcription(op, run)
    assert n >= sum(c.n_edge - len(c.no_ref) for c in ki.cases(op))
    kat_refs.assert_coverage(op, kat_refs.run_all(op, run))


@pytest.mark.parametrize("op", sorted(kat_refs.NO_TRANSCRIPTION))
def test_host_build_reaches_the_edges_of_the_untranscribed_ops(art, op):
    run = kat_refs.host_runner(art, op)
    kat_refs.assert_coverage(op, kat_refs.run_all(op, run))


# ------------------------------------------------------------------------------------------------ mpmath
def mpf(x):
    return libmp.from_float(float(x))


def round_f32(v):
    """the binary32 nearest to the mpf v (ties to even), denormals and overflow included, as a Python float"""
    sign, man, exp, bc = v
    if man == 0:
        return 0.0
    e = exp + bc - 1                                   # 2^e <= |v| < 2^(e + 1)
    if e >= 128:
        return -np.inf if sign else np.inf
    prec = 24 if e >= -126 else e + 150                # denormals keep fewer bits
    if prec <= 0:
        r = 2.0 ** -149 if (prec == 0 and man != 1) else 0.0      # above half the smallest denormal / at or below it (the tie goes to even: 0)
        return -r if sign else r
    r = libmp.to_float(libmp.mpf_pos(v, prec, RND))
    return float(np.float32(r))                        # exact, or 2^128 -> inf


def ulp_distance(a, b):
    """distance in units of the last place between binary32 arrays (NaN: huge)"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    return np.where(np.isnan(a) | np.isnan(b), 1 << 40, d)


def report(name, got, want):
    d = ulp_distance(got.astype(np.float32), want.astype(np.float32))
    zero = (got == 0) & (want == 0)                    # +0 and -0 are the same number: ART-M1 has no signed-zero contract (tests/kat_inputs.py sincos_case)
    d = np.where(zero, 0, d)
    print("%s: %d items, %d not correctly rounded, max distance %d ulp" % (name, got.size, int((d != 0).sum()), int(d.max())))
    return d


def test_sin_cos_tan_are_correctly_rounded(art):
    case, = ki.cases("sincos")
    sc = devkat.run_host(art, "sincos", case.words).view(np.float32)
    tn = devkat.run_host(art, "tan", case.words).view(np.float32)
    ws, wc, wt = [], [], []
    for x in case.inp[:, 0]:
        c, s = libmp.mpf_cos_sin(mpf(x), PREC, RND)
        ws.append(round_f32(s)); wc.append(round_f32(c)); wt.append(round_f32(libmp.mpf_div(s, c, PREC, RND)))
    for name, got, want in [("sin", sc[:, 0], np.array(ws)), ("cos", sc[:, 1], np.array(wc)), ("tan", tn[:, 0], np.array(wt))]:
        d = report(name, got, want)
        assert d.max() <= 1, "%s: more than 1 ulp from the true value at x = %r" % (name, float(case.inp[int(d.argmax()), 0]))
        assert (d != 0).sum() == 0, "%s: not the correctly rounded value at %s" % (name, [float(v).hex() for v in case.inp[np.flatnonzero(d)[:8], 0]])
    # safe_tan: tan but for +-kHalfPi, where vector_math.adb:14-22 returns Float'Last
    half = np.abs(case.inp[:, 0]) == ki.HALF_PI
    assert half.sum() >= 2 and np.all(tn[half, 1] == ki.FLT_MAX) and np.array_equal(tn[~half, 1].view(np.uint32), tn[~half, 0].view(np.uint32))


def test_apow_is_correctly_rounded(art):
    case, = ki.cases("apow")
    got = devkat.run_host(art, "apow", case.words).view(np.float32)[:, 0]
    x, y = case.inp[:, 0], case.inp[:, 1]
    general = (x > 0) & np.isfinite(x) & ~np.isnan(y)                  # the rest: RM A.5.1 special cases, held to the transcription and the list below
    want = np.zeros(x.size)
    for i in np.flatnonzero(general):
        want[i] = round_f32(libmp.mpf_pow(mpf(x[i]), mpf(y[i]), PREC, RND))
    d = report("apow", got[general], want[general])
    assert d.max() <= 1, "apow: more than 1 ulp from the true value"
    bad = np.flatnonzero(general)[np.flatnonzero(d)]
    assert bad.size == 0, "apow: not the correctly rounded value at %s" % [(float(x[i]).hex(), float(y[i]).hex()) for i in bad[:8]]
    nan, inf = np.isnan(got), np.isinf(got)
    assert np.all(nan[np.isnan(x) | np.isnan(y) | (x < 0) | ((x == 0) & (y == 0))])
    assert np.all(got[(x == 0) & (y > 0)] == 0) and np.all(inf[(x == 0) & (y < 0)])
    pinf = np.isinf(x) & (x > 0) & ~np.isnan(y)
    assert np.all(got[pinf & (y == 0)] == 1) and np.all(inf[pinf & (y > 0)]) and np.all(got[pinf & (y < 0)] == 0)


def rel_error_log2(got, want):
    """log2 of the largest |got - want| / |want| (got: binary64 array, want: list of mpf)"""
    worst = libmp.fzero
    for g, w in zip(got, want):
        if w[1] == 0:
            assert g == 0.0
            continue
        e = libmp.mpf_abs(libmp.mpf_div(libmp.mpf_sub(libmp.from_float(float(g)), w, PREC, RND), w, PREC, RND))
        if libmp.mpf_gt(e, worst):
            worst = e
    return float(libmp.to_float(libmp.mpf_log(worst, 53, RND))) / np.log(2.0) if worst[1] else -np.inf


def as_f64(words):
    return np.ascontiguousarray(words).view(np.float64)[:, 0]


def test_log_pos_and_exp_small_hold_two_to_the_minus_fifty(art):
    """the polynomial lengths of art_math.h were chosen for 2^-50 relative error of the binary64 intermediate: what the single rounding
    to binary32 of apow rests on"""
    case, = ki.cases("log_pos")
    got = as_f64(devkat.run_host(art, "log_pos", case.words))
    keep = case.inp[:, 0] != 1                                          # log 1 = 0 exactly: checked by rel_error_log2's zero branch
    e_log = rel_error_log2(got, [libmp.mpf_log(mpf(x), PREC, RND) if x != 1 else libmp.fzero for x in case.inp[:, 0]])
    case, = ki.cases("exp_small")
    got = as_f64(devkat.run_host(art, "exp_small", case.words))
    e_exp = rel_error_log2(got, [libmp.mpf_exp(mpf(t), PREC, RND) for t in case.inp[:, 0]])
    print("log_pos: max relative error 2^%.2f on %d items; exp_small: 2^%.2f on %d items" % (e_log, int(keep.sum()), e_exp, got.size))
    assert e_log < -50 and e_exp < -50
