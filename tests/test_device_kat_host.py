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

import ada_transcription as ada
import devkat
import kat_inputs as ki
import kat_refs

PREC = 120
RND = "n"
TRANSCRIBED = [op for op in devkat.OPS if not (op in kat_refs.NO_TRANSCRIPTION and kat_refs.NO_TRANSCRIPTION[op] is not None)]


@pytest.mark.parametrize("op", TRANSCRIBED)
def test_host_build_equals_the_transcription(art, op):
    """For camera_dir and resolve also the float64 references below (assert_float64): the host build within twice the transcription's own
    deviation from them, as tests/test_gpu_device_kat.py asks of the device build.  Measured on the sets of tests/kat_inputs.py:
      camera_dir  369 920 items in 272 Cases, measured and allowed per Case (frame, matrix, cam_z, AA): the transcription's largest component
                  deviation from float64 runs from 0 (1x1 without AA: the ray is the axis) to 2.5282e-06 (a rotation with a translation
                  that nearly cancels the ray), allowed twice the Case's own value, 0 to 5.0564e-06;
      resolve     154 770 items: the transcription's product deviates from 255 min(sqrt(a norm), 1) in float64 by at most 1.9437e-05,
                  allowed margin around a tie 3.8874e-05; 2 284 items (1.48 %) have a byte one off the float64 byte, all of them inside the
                  transcription's own margin; allowed 2 %."""
    run = kat_refs.host_runner(art, op)
    n = kat_refs.assert_matches_transcription(op, run)
    assert n >= sum(c.n_edge - len(c.no_ref) for c in ki.cases(op))
    kat_refs.assert_coverage(op, kat_refs.run_all(op, run))
    assert_float64(op, run)
    if op == "resolve":
        assert_resolve_is_the_oracles(run)


@pytest.mark.parametrize("op", sorted(kat_refs.NO_TRANSCRIPTION))
def test_host_build_reaches_the_edges_of_the_untranscribed_ops(art, op):
    run = kat_refs.host_runner(art, op)
    kat_refs.assert_coverage(op, kat_refs.run_all(op, run))


# ------------------------------------------------------------------------------------------------ float64 references
def camera_f64(case):
    """normalize(M normalize(r)) in float64, M applied as a point transform; the jitter offsets are thirds, not their binary32 roundings"""
    d = case.pdesc
    W, H = d["width"], d["height"]
    pix, smp = case.words[:, 0].astype(np.int64), case.words[:, 1].astype(np.int64)
    x, y = (pix % W).astype(np.float64), (pix // W).astype(np.float64)
    if d["aa_on"]:
        ox, oy = (1 + ((smp >> 1) & 1)) / 3.0, (1 + (smp & 1)) / 3.0
    else:
        ox = oy = 0.5
    r = np.stack([x + ox - W / 2.0, y + oy - H / 2.0, np.full(x.shape, float(d["cam_z"]))], axis=1)
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    M = np.array(d["matrix"], np.float64)
    v = r @ M[:3, :3].T + M[:3, 3]
    return v / np.linalg.norm(v, axis=1, keepdims=True)


_camera_dev = {}


def camera_deviation(words, case):
    return float(np.abs(words.view(np.float32).astype(np.float64) - camera_f64(case)).max())


def camera_transcription_deviation():
    """per Case the largest |component of the binary32 transcription - float64| over every item: computed once"""
    if not _camera_dev:
        _camera_dev.update({c.label: camera_deviation(kat_refs.camera_expected(c, c.inp.shape[0]), c) for c in ki.cases("camera_dir")})
    return _camera_dev


def resolve_f64(case):
    """per channel 255 min(sqrt(a norm), 1) in float64 and whether it is defined (a norm >= 0, no NaN)"""
    a, norm = case.inp[:, :3].astype(np.float64), case.inp[:, 3:4].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = a * norm
        ok = t >= 0
        p = 255.0 * np.minimum(np.sqrt(np.where(ok, t, 0.0)), 1.0)
    return p, ok


def half_up(p):
    return np.floor(p + 0.5).astype(np.int64)


def unpack(words):
    w = words[:, 0].astype(np.int64)
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], axis=1)


_resolve_dev = []


def resolve_transcription_deviation():
    """(margin, items one off, items): the transcription against float64 over the whole resolve Case -- the largest deviation of the binary32
    product that is converted, and the items whose byte is not the float64 byte.  The transcription runs on every item here, not on the
    first thousand random ones only; computed once."""
    if not _resolve_dev:
        case, = ki.cases("resolve")
        p, ok = resolve_f64(case)
        with np.errstate(all="ignore"):
            # the transcription's operations on binary32 arrays -- the same operation per element; "**" with 0.5 is sqrt but for x = 0 and 1,
            # which sqrt maps to themselves (-0 to +0 by the x = 0 case) -- checked against the scalar text on the items it runs on
            x = case.inp[:, 3:4] * case.inp[:, :3]
            s = np.where(x == 0, np.float32(0), np.sqrt(x))
            v32 = np.where(s < 1, s, np.float32(1)) * np.float32(255)
            b = np.where(v32 > 0, np.floor(v32.astype(np.float64) + 0.5), 0).astype(np.int64)
            m = case.n_transcribed()
            sv = np.array([[ada.resolve_channel(a, row[3]) for a in row[:3]] for row in case.inp[:m]], np.float32)
            sb = np.array([[ada.to_unsigned_32(c) for c in row] for row in sv], np.int64)
        assert np.array_equal(sv, v32[:m], equal_nan=True) and np.array_equal(sb, b[:m])
        v = v32.astype(np.float64)
        margin = float(np.abs(v - p)[ok].max())
        off = compare_bytes("the transcription", case, b, margin, margin)
        _resolve_dev.append((margin, off, case.inp.shape[0]))
    return _resolve_dev[0]


def compare_bytes(who, case, got, margin_measured, margin_allowed):
    """got [n, 3] bytes against the float64 reference: equal, or one off where the float64 product lies within margin_allowed of a tie.
    Returns the number of items with a byte that is one off."""
    p, ok = resolve_f64(case)
    want = half_up(p)
    near = np.abs(p - np.floor(p) - 0.5) <= margin_allowed
    diff = np.abs(got - want)
    bad = ok & ~((diff == 0) | ((diff == 1) & near))
    i = np.flatnonzero(bad.any(axis=1))
    assert i.size == 0, "resolve: %s differs from the float64 reference outside the tie margin %.4e on %d items, first: item %d in %s got %s want %s" % (
        who, margin_allowed, i.size, i[0], case.inp[i[0]].tolist(), got[i[0]].tolist(), want[i[0]].tolist())
    return int((ok & (diff == 1)).any(axis=1).sum())


MAX_ONE_OFF = 0.02              # of the items


def assert_float64(op, run):
    """run(case) -> the output words of one build.  camera_dir: every component within twice the transcription's own deviation from the
    float64 ray.  resolve: every byte the float64 byte, but within twice the transcription's margin of a tie one off; under 2 % of the items."""
    if op == "camera_dir":
        measured = camera_transcription_deviation()
        got = {c.label: camera_deviation(run(c), c) for c in ki.cases(op)}
        print("camera_dir: %d items in %d Cases; per Case the transcription deviates from float64 by at most %.4e .. %.4e, allowed twice that: %.4e .. %.4e; this build: %.4e .. %.4e" % (
            sum(c.inp.shape[0] for c in ki.cases(op)), len(got), min(measured.values()), max(measured.values()), 2 * min(measured.values()), 2 * max(measured.values()),
            min(got.values()), max(got.values())))
        over = [k for k in got if not got[k] <= 2 * measured[k]]
        assert not over, "camera_dir: %d Cases deviate from the float64 ray by more than twice the transcription's own deviation, first %s: %.4e against %.4e" % (
            len(over), over[0], got[over[0]], measured[over[0]])
    elif op == "resolve":
        case, = ki.cases(op)
        margin, t_off, n = resolve_transcription_deviation()
        off = compare_bytes("this build", case, unpack(run(case)), margin, 2 * margin)
        print("resolve: %d items; the transcription's product deviates from float64 by at most %.4e, allowed tie margin %.4e; one off the float64 byte: "
              "the transcription %d items (%.2f %%), this build %d items (%.2f %%), allowed %.0f %%" % (n, margin, 2 * margin, t_off, 100.0 * t_off / n, off, 100.0 * off / n, 100 * MAX_ONE_OFF))
        assert t_off < MAX_ONE_OFF * n and off < MAX_ONE_OFF * n


def assert_resolve_is_the_oracles(run):
    """orc.resolve on the same sums, bit for bit, per spp (the oracle takes the integer, norm_c is its 1 / spp)"""
    import orc
    case, = ki.cases("resolve")
    got = run(case)[:, 0]
    seen = 0
    for spp in ki.RESOLVE_SPPS:
        m = case.words[:, 3] == (np.float32(1) / np.float32(spp)).view(np.uint32)
        want = orc.resolve(np.ascontiguousarray(case.inp[m, :3]).reshape(1, -1, 3), spp).reshape(-1)
        bad = np.flatnonzero(got[m] != want)
        assert bad.size == 0, "resolve: spp %d: %d of %d items differ from orc.resolve, first %s got %#x want %#x" % (
            spp, bad.size, int(m.sum()), case.inp[m][bad[0]].tolist(), int(got[m][bad[0]]), int(want[bad[0]]))
        seen += int(m.sum())
    assert seen == case.inp.shape[0]


def test_the_transcription_alone_meets_the_coverage_and_the_cap():
    """No build at all: the boundary lists of tests/kat_inputs.py, run through the transcription, reach both sides of at least 250 of the
    255 rounding boundaries (measured: 255 of 255 for ada_round_u32 and for every norm_c of the resolve), and the transcription's bytes stay
    under the 2 % cap against the float64 reference.  mpmath at 120 bits agrees with the float64 reference on every edge item."""
    with np.errstate(all="ignore"):
        case, = ki.cases("round_u32")
        out = np.array([[ada.to_unsigned_32(v)] for v in case.inp[:, 0]], np.int64).astype(np.uint32)
        n_round = kat_refs.assert_boundary_coverage("round_u32", case, out)
        case, = ki.cases("resolve")
        out = np.array([[ada.resolve(tuple(row[:3]), row[3])] for row in case.inp], np.int64).astype(np.uint32)
        n_res = kat_refs.assert_boundary_coverage("resolve", case, out)
    margin, off, n = resolve_transcription_deviation()
    print("boundaries with both sides present: round_u32 %d, resolve %d (the least over the norm_c) of 255; one off the float64 byte: %d of %d items (%.2f %%)" % (n_round, n_res, off, n, 100.0 * off / n))
    assert off < MAX_ONE_OFF * n
    exact = sum(1 for spp in ki.RESOLVE_SPPS for w in ki.RESOLVE_RISES[spp] if ada.resolve_channel(np.uint32(w).view(np.float32), np.float32(1) / np.float32(spp)) % 1 == 0.5)
    print("resolve: %d of %d rises land on k + 0.5 exactly" % (exact, 255 * len(ki.RESOLVE_SPPS)))
    assert exact > 0
    p, ok = resolve_f64(case)
    worst = 0.0
    for i in range(case.n_edge):
        for c in range(3):
            if not ok[i, c] or not np.isfinite(case.inp[i, c]): continue
            t = libmp.mpf_mul(mpf(case.inp[i, c]), mpf(case.inp[i, 3]), PREC, RND)
            s = libmp.mpf_sqrt(t, PREC, RND)
            if libmp.mpf_gt(s, libmp.fone): s = libmp.fone
            worst = max(worst, abs(libmp.to_float(libmp.mpf_mul(s, libmp.from_int(255), PREC, RND)) - p[i, c]))
    print("resolve: float64 against mpmath on the %d edge items: %.3e" % (case.n_edge, worst))
    assert worst < 1e-12


def test_the_inputs_name_the_reference_camera(art):
    from ada_ray_tracer_amd import scenes
    assert tuple(ki.REFERENCE_CAMERA) == tuple(scenes.REFERENCE_CAMERA)


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
