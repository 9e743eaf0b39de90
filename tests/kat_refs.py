"""What the independent Ada transcription (tests/ada_transcription.py) says an item of a known-answer op must give, in the op's output
layout (tests/device_kat/kat_ops.h), and the comparison shared by tests/test_gpu_device_kat.py and tests/test_device_kat_host.py.
expect(op, case, i) returns (words, columns): the expected output words of item i and the columns the transcription defines
(a rejected triangle has no t, u, v in the Ada text), or None where it defines nothing."""
import numpy as np

import ada_transcription as ada
import devkat
import kat_inputs as ki

f = np.float32
T = lambda a: tuple(f(c) for c in a)
NO_TRANSCRIPTION = {"tan": "the Ada text calls the run-time library's Tan; mpmath checks atan_m1 on the CPU",
                    "sqrt": None, "rcp": None, "div": None, "colour_lum": None,      # numpy's own binary32 operations ARE the reference: see expect()
                    "sincos_f64": "ART-M1 internals: the binary64 sine and cosine before the single rounding, host build only",
                    "log_pos": "ART-M1 internals: checked against mpmath on the CPU", "exp_small": "ART-M1 internals: checked against mpmath on the CPU",
                    "slab": "this backend's own slab arithmetic, not reference code: host build only"}


def _w(vals):
    return np.array([np.float32(v) for v in vals], np.float32).view(np.uint32)


def _key(k):
    return np.uint32(k).view(np.float32)


def _mat_sample(m, x1, x2, d, n):
    p = m["p"]
    if m["type"] == ki.MAT_LAMBERT: return ada.lambert_sample(T(p[:3]), x1, x2, d, n)
    if m["type"] == ki.MAT_MIRROR: return ada.mirror_sample(T(p[:3]), d, n)
    if m["type"] == ki.MAT_GLASS: return ada.glass_sample(T(p[:3]), T(p[3:6]), p[6], x1, d, n)
    return ada.phong_sample(T(p[:3]), p[3], x1, x2, d, n)


def _mat_eval(m, l, v, n):
    p = m["p"]
    if m["type"] == ki.MAT_LAMBERT: return ada.lambert_eval(T(p[:3]), l, v, n)
    if m["type"] == ki.MAT_PHONG: return ada.phong_eval(T(p[:3]), p[3], l, v, n)
    return ada.V(0, 0, 0), f(1)


def expect(op, case, i):
    x = [f(v) for v in case.inp[i]]
    L = case.pdesc
    if op == "sincos": return _w([ada.sin(x[0]), ada.cos(x[0])]), None
    if op == "apow": return _w([ada.ada_pow(x[0], x[1])]), None
    if op == "sqrt": return _w([np.sqrt(x[0])]), None
    if op == "rcp": return _w([f(1) / x[0]]), None
    if op == "div": return _w([x[0] / x[1]]), None
    if op == "normalize": return _w(ada.normalize(T(x))), None
    if op == "reflect": return _w(ada.reflect(T(x[:3]), T(x[3:]))), None
    if op == "perpendicular": return _w(ada.get_perpendicular(T(x))), None
    if op == "sample_cosine": return _w(ada.map_sample_to_cosine_dist(x[0], x[1], T(x[2:5]), T(x[5:8]), x[8])), None
    if op == "sample_cosine_fixed": return _w(ada.map_sample_to_cosine_dist_fixed(x[0], x[1], T(x[2:5]), T(x[5:8]), x[8])), None
    if op == "fresnel": return _w([ada.fresnel(x[0], x[1], x[2])]), None
    if op == "light_sample":
        r = ada.sphere_light_sample(L, x[0], x[1], T(x[2:])) if L["shape"] == 1 else ada.area_light_sample(L, x[0], x[1], T(x[2:]))
        return _w(list(r["pos"]) + list(r["dir"]) + list(r["intensity"]) + [r["pdf"]]), None
    if op == "light_eval_pdf":
        return _w([ada.sphere_light_eval_pdf(L, T(x[:3])) if L["shape"] == 1 else ada.area_light_eval_pdf(L, T(x[:3]), T(x[3:6]), x[6])]), None
    if op == "sphere_light_pdf": return _w([ada.sphere_light_eval_pdf(L, T(x))]), None
    if op == "pdf_area_to_solid": return _w([ada.pdf_a_to_w(x[0], x[1], x[2])]), None
    if op == "bsdf_sample":
        r = _mat_sample(L, x[0], x[1], T(x[2:5]), T(x[5:8]))
        return _w(list(r["color"]) + list(r["dir"]) + [r["pdf"], 1.0 if r["specular"] else 0.0]), None
    if op == "bsdf_eval":
        b, p = _mat_eval(L, T(x[:3]), T(x[3:6]), T(x[6:9]))
        return _w(list(b) + [p]), None
    if op == "tri_raw":
        h = ada.intersect_triangle(T(x[:3]), T(x[3:6]), T(x[6:9]), T(x[9:12]), T(x[12:15]), f(-np.inf), f(np.inf))
        if h["is_hit"]: return _w([h["tmin"], h["u"], h["v"], 1.0]), None
        return _w([0, 0, 0, 0.0]), [3]                                   # (a NaN or infinite t fails the Ada text's window test t_min < t < t_max: assert_matches_transcription)
    if op == "sphere":
        h = ada.intersect_all_spheres(T(x[:3]), T(x[3:6]), [(T(x[6:9]), x[9], 0)])
        return (_w([h["t"], _key(ki.KEY_SPHERE)]), None) if h["is_hit"] else (_w([ki.FLT_MAX, _key(ki.KEY_MISS)]), None)
    if op == "cornell":
        hit, tmin, tmax = ada.intersect_box(T(x[:3]), T(x[3:6]), L["min"], L["max"])
        h = ada.intersect_cornell(T(x[:3]), T(x[3:6]), L)
        # (scene.adb:73 keeps a hit only if t < Float'Last: a Cornell "hit" at t = inf -- a zero direction -- is none; the product's candidate says so at once)
        tail = [h["t"], _key(ki.KEY_CORNELL | h["prim"][1])] if h["is_hit"] and h["t"] < ki.FLT_MAX else [ki.FLT_MAX, _key(ki.KEY_MISS)]
        return _w([1.0 if hit else 0.0, tmin, tmax] + tail), None
    if op == "quad":
        h = ada.intersect_flat_light(T(x[:3]), T(x[3:6]), L)
        return (_w([h["t"], _key(ki.KEY_QUAD)]), None) if h["is_hit"] else (_w([ki.FLT_MAX, _key(ki.KEY_MISS)]), None)
    if op == "resolve": return np.array([ada.resolve(T(x[:3]), x[3])], np.uint32), None
    if op == "round_u32": return np.array([ada.to_unsigned_32(x[0])], np.uint32), None
    if op == "colour_lum": return _w([(f(0.2126) * x[0] + f(0.7152) * x[1]) + f(0.0722) * x[2]]), None      # include/art_hip.h, art_bind_moments: binary32, not contracted
    if op == "cand_wins":
        w = case.words[i]
        t, bt = x[0], x[2]
        return _w([1.0 if (t < bt) or (t == bt and w[3] != ki.KEY_MISS and w[1] < w[3]) else 0.0]), None
    return None


def camera_expected(case, n):
    """camera_dir of the first n items of a camera Case, all at once: the transcription's functions on binary32 arrays, which are the same
    binary32 operations per element.  Sample s takes res(s mod 4) of Generate4RayDirections; without AA every sample is EyeRayDirection."""
    d = case.pdesc
    W, H = d["width"], d["height"]
    pix, smp = case.words[:n, 0].astype(np.int64), case.words[:n, 1].astype(np.int64)
    x, y = pix % W, pix // W
    if d["aa_on"]:
        off = np.array(ada.AA_OFFSETS, np.float32)[smp % 4]
        ox, oy = off[:, 0], off[:, 1]
    else:
        ox = oy = f(0.5)
    r = ada.eye_ray_direction(x, y, ox, oy, W, H, d["cam_z"])
    out = ada.normalize(ada.mat_mul_point(d["matrix"], r))
    return np.stack([np.broadcast_to(c, (n,)) for c in out], axis=1).astype(np.float32).view(np.uint32)


_expected = {}


class ArgumentError(Exception):
    pass


def _strict_pow(x, y):
    """Vector_Math.pow with the exceptions of the Ada text (vector_math.adb:27-35), which the transcription's ada_pow leaves out: such an
    item has no defined answer there (the product returns a quiet NaN, or +inf for 0 ** negative) and is compared with the host build only"""
    if (x == 0 and y <= 0) or x < 0:
        raise ArgumentError("pow(%r, %r)" % (x, y))
    return _ada_pow(x, y)


_ada_pow = ada.ada_pow
RAISING_SETS = {"phong_0"}            # cosPower 0: a lobe cosine clamped to 0 is 0 ** 0 (tests/kat_inputs.py material_sets)


def _transcribe_case(op, case):
    if op == "camera_dir":
        n = case.n_transcribed()
        return case, np.arange(n), camera_expected(case, n), np.ones((n, 3), bool)
    idx, rows, masks = [], [], []
    for i in range(case.n_transcribed()):
        if i in case.no_ref:
            continue
        try:
            words, cols = expect(op, case, i)
        except ArgumentError:
            assert case.label in RAISING_SETS, (op, case.label, i)
            continue
        m = np.ones(words.size, bool)
        if cols is not None:
            m[:] = False; m[cols] = True
        idx.append(i); rows.append(words); masks.append(m)
    return case, np.array(idx), np.array(rows, np.uint32), np.array(masks)


def expected_table(op):
    """[(case, item indices, expected words, column mask)] for the edge list and the first N_TRANSCRIBED_RANDOM random items of every Case
    of op: computed once per process and shared"""
    if op not in _expected:
        _expected[op] = []
        if NO_TRANSCRIPTION.get(op) is None:
            ada.ada_pow = _strict_pow
            try:
                with np.errstate(all="ignore"):
                    _expected[op] = [_transcribe_case(op, case) for case in ki.cases(op)]
            finally:
                ada.ada_pow = _ada_pow
    return _expected[op]


def differing(op, got, want, mask=None):
    """items of got (n x words) that differ from want under the rule: both NaN, or the same bits (binary64 halves: the same bits)"""
    if op in ("log_pos", "exp_small", "sincos_f64", "resolve", "round_u32"):      # (and integers: the same bits)
        bad = got != want
    else:
        bad = ~((got == want) | (np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))))
    if mask is not None:
        bad &= mask
    return np.flatnonzero(bad.any(axis=1))


def assert_matches_transcription(op, run):
    """run(case) -> output words of the whole case; every transcribed item must match"""
    n = 0
    for case, idx, want, mask in expected_table(op):
        got = run(case)[idx]
        if op == "tri_raw":                                              # the Ada text rejects a triangle whose t is NaN or infinite by its window test, which tri_raw leaves to its caller
            mask = mask & ~((want[:, 3] == 0) & ~np.isfinite(got[:, 0].view(np.float32)))[:, None]
        bad = differing(op, got, want, mask)
        assert bad.size == 0, "%s/%s: %d of %d items differ from the Ada transcription, first: item %d in %s got %s want %s" % (
            op, case.label, bad.size, idx.size, idx[bad[0]], case.inp[idx[bad[0]]].tolist(), got[bad[0]].view(np.float32).tolist(), want[bad[0]].view(np.float32).tolist())
        n += idx.size
    return n


# ------------------------------------------------------------------------------------------------ coverage: were the edges reached?
def assert_coverage(op, outputs):
    """outputs: [(case, output words)] of one side.  Asserts, from inputs and outputs, that the op's branches all occurred."""
    fl = lambda w: w.view(np.float32)
    _assert_picture_ends_coverage(op, outputs)
    if op == "bsdf_sample":
        seen = set(); tir = 0
        for case, out in outputs:
            if case.pdesc["type"] != ki.MAT_GLASS: continue
            d, n, o = case.inp[:, 2:5], case.inp[:, 5:8], fl(out)
            din = np.einsum("ij,ij->i", d, n); dout = np.einsum("ij,ij->i", o[:, 3:6], n)
            ok = np.isfinite(dout) & (din != 0)
            seen |= set(zip((din[ok] < 0).tolist(), (dout[ok] * din[ok] > 0).tolist()))
            # total internal reflection: the refraction branch was drawn (xi1 = 0 <= k_trans) yet the ray came back to its own side
            ior = float(case.pdesc["p"][6]); eta = np.where(-din < 0, 1.0 / ior, ior)
            tir += int(np.count_nonzero(ok & (case.inp[:, 0] == 0) & (1.0 - (1.0 - din.astype(np.float64) ** 2) / eta ** 2 < -1e-6) & (dout * din < 0)))
        assert len(seen) == 4, "glass: entering / leaving x reflected / refracted must all occur: %s" % seen
        assert tir > 0, "glass: total internal reflection must occur"
    elif op == "apow":
        (case, out), = outputs
        x, y = case.inp[:, 0].astype(np.float64), case.inp[:, 1].astype(np.float64)
        with np.errstate(all="ignore"):
            t = y * np.log(x)
        gen = (x > 0) & (x != 1) & np.isfinite(x) & (y != 0) & (y != 1) & (y != 2) & (y != 0.5) & ~np.isnan(y)
        for name, m in [("NaN operand", np.isnan(x) | np.isnan(y)), ("0 ** 0", (x == 0) & (y == 0)), ("negative base", x < 0), ("y = 0", (x > 0) & (y == 0)),
                        ("0 ** negative", (x == 0) & (y < 0)), ("0 ** positive", (x == 0) & (y > 0)), ("x = 1", (x == 1) & (y != 0)), ("y = 1", (x > 0) & (x != 1) & (y == 1)),
                        ("y = 2", (x > 0) & (x != 1) & (y == 2)), ("y = 0.5", (x > 0) & (x != 1) & (y == 0.5)), ("x = inf", np.isinf(x) & (x > 0) & (y != 0) & (y != 1) & (y != 2) & (y != 0.5) & ~np.isnan(y)),
                        ("upper clamp", gen & (t > 200) & (t < 200.001)), ("just below the upper clamp", gen & (t < 200) & (t > 199.999)),
                        ("lower clamp", gen & (t < -200) & (t > -200.001)), ("just above the lower clamp", gen & (t > -200) & (t < -199.999)),
                        ("general case", gen & (np.abs(t) < 100))]:
            assert m.any(), "apow: no item takes the case '%s'" % name
    elif op == "tri_raw":
        (case, out), = outputs
        o = fl(out); t, u, v, acc = o[:, 0], o[:, 1], o[:, 2], o[:, 3]
        with np.errstate(all="ignore"):
            a, b, c = v > 0, u > 0, (u + v).astype(np.float32) < 1
        assert np.array_equal(acc == 1, a & b & c), "accepted is not (v > 0, u > 0, u + v < 1) of the returned u, v"
        for name, m in [("v > 0 fails", ~a), ("v > 0 holds, u > 0 fails", a & ~b), ("v, u > 0 hold, u + v < 1 fails", a & b & ~c), ("accepted", a & b & c)]:
            assert m[:case.n_edge].any() and m[case.n_edge:].any(), "triangles: '%s' must occur among the edges and among the random items" % name
    elif op == "cornell":
        (case, out), = outputs
        keys = out[:, 4]
        for p in range(5):
            assert (keys == (ki.KEY_CORNELL | p)).any(), "Cornell box: plane %d never hit" % p
        assert ((fl(out)[:, 0] == 1) & (keys == ki.KEY_MISS)).any(), "Cornell box: no ray left through the open face"
    elif op == "sincos":
        (case, out), = outputs
        with np.errstate(all="ignore"):
            k = np.rint(case.inp[:case.n_edge, 0].astype(np.float64) * (2 / np.pi)).astype(int)
        assert set(range(-9, 10)) <= set(k.tolist()), "sincos: every k of -9..9 must occur among the edges"
    elif op == "cand_wins":
        (case, out), = outputs
        w = fl(out)[:, 0]
        tie = case.words[:, 0] == case.words[:, 2]
        assert (w[tie] == 1).any() and (w[tie] == 0).any() and (w[~tie] == 1).any() and (w[~tie] == 0).any()
    elif op in ("sphere", "quad"):
        (case, out), = outputs
        hit = out[:, 1] != ki.KEY_MISS
        assert hit[:case.n_edge].any() and (~hit[:case.n_edge]).any() and hit[case.n_edge:].any() and (~hit[case.n_edge:]).any()
    elif op == "slab":
        (case, out), = outputs
        o = fl(out)
        with np.errstate(all="ignore"):
            hit = o[:, 6] <= o[:, 7]
        assert hit.any() and (~hit).any() and (np.abs(o[:case.n_edge, 0]) == f(1) / f(1e-30)).any(), "slab: hits, misses and the 1e-30 clamp must occur"
    elif op == "fresnel":
        (case, out), = outputs
        F = fl(out)[:, 0]
        assert (F[:case.n_edge] == 1).any() and ((F[:case.n_edge] > 0) & (F[:case.n_edge] < 1)).any(), "fresnel: total reflection and partial reflection at the edges"
    elif op in ("light_sample", "sphere_light_pdf", "light_eval_pdf"):
        for case, out in outputs:
            L = case.pdesc
            if L["shape"] != 1: continue
            p = case.inp[:, 2:5] if op == "light_sample" else case.inp[:, :3]
            d2 = ((p - np.array(L["center"], np.float32)) ** 2).sum(axis=1)
            inside = d2 - float(L["radius"]) ** 2 < 1e-4
            assert inside[:case.n_edge].any() and (~inside[:case.n_edge]).any() and inside[case.n_edge:].any(), "sphere light: points inside and outside"


MIN_BOUNDARIES = 250            # of the 255 rises of the byte, both sides must occur among the inputs


def boundaries_reached(in_words, out_bytes):
    """the bytes k for which two inputs one ulp apart (positive, finite) give k and k + 1"""
    keep = in_words < 0x7F800000
    w, first = np.unique(in_words[keep], return_index=True)
    b = out_bytes[keep][first].astype(np.int64)
    adj = (w[1:].astype(np.int64) == w[:-1].astype(np.int64) + 1) & (b[1:] == b[:-1] + 1)
    return set(b[:-1][adj].tolist())


def assert_boundary_coverage(op, case, out):
    """resolve: per norm_c, on the red channel; round_u32: on its one input"""
    if op == "round_u32":
        groups = [("", case.words[:, 0], out[:, 0])]
    else:
        groups = [("norm_c %r: " % float(np.uint32(nw).view(np.float32)), case.words[case.words[:, 3] == nw, 0], out[case.words[:, 3] == nw, 0] & 255)
                  for nw in np.unique(case.words[:case.n_edge, 3])]
    for name, w, b in groups:
        got = boundaries_reached(w, b) & set(range(255))
        assert len(got) >= MIN_BOUNDARIES, "%s: %sboth sides of only %d of the 255 rounding boundaries occur" % (op, name, len(got))
    return min(len(boundaries_reached(w, b) & set(range(255))) for _, w, b in groups)


def _assert_picture_ends_coverage(op, outputs):
    fl = lambda w: w.view(np.float32)
    if op in ("resolve", "round_u32"):
        (case, out), = outputs
        assert_boundary_coverage(op, case, out)
        edge = out[:case.n_edge, 0]
        top = (edge == 0x00FFFFFF) if op == "resolve" else (edge == int(ki.ROUND_TOP))
        assert top.any() and (edge == 0).any(), "%s: the two ends of the range must occur among the edges" % op
    elif op == "camera_dir":
        for case, out in outputs:
            d = case.pdesc
            pix, smp = case.words[:case.n_edge, 0], case.words[:case.n_edge, 1]
            assert (pix == 0).any() and (pix == d["width"] * d["height"] - 1).any(), "camera: the first and the last pixel must occur"
            first = out[:case.n_edge][pix == 0]
            distinct = len({tuple(r) for r in first.tolist()})
            assert (smp[pix == 0] >= 4).any() and distinct == (4 if d["aa_on"] else 1), "camera/%s: pixel 0 has %d distinct rays" % (case.label, distinct)
            assert np.isfinite(fl(out)).all(), "camera/%s: a ray is not finite" % case.label


def run_all(op, run):
    return [(case, run(case)) for case in ki.cases(op)]


def host_runner(art, op):
    cache = {}

    def run(case):
        if id(case) not in cache:
            cache[id(case)] = devkat.run_host(art, op, case.words, case.params)
        return cache[id(case)]
    return run
