"""Inputs of the per-function known-answer tests (tests/test_gpu_device_kat.py on the GPU, tests/test_device_kat_host.py on the CPU): for every
op of tests/device_kat/kat_ops.h a list of Cases.  A Case is one launch: an optional parameter record (a light, a material, the Cornell
box) and an array of items -- first an EDGE LIST of explicit values chosen where the arithmetic can go wrong, then a SEEDED RANDOM FILL.
Everything is deterministic; nothing here looks at what the code under test returns.

`Case.no_ref` names the edge items for which the Ada transcription (tests/ada_transcription.py) has no defined answer, with the reason;
those are compared with the host build only.  One set raises in the Ada text itself: with cosPower 0 (material set phong_0) a lobe cosine
clamped to 0 is pow(0, 0), Argument_Error in vector_math.adb:27; tests/kat_refs.py skips exactly the items of that set that raise."""
import struct

import numpy as np

import ada_transcription as ada

f = np.float32
SEED = 0xD0E5
INF = f(np.inf)
NAN = f(np.nan)
FLT_MAX = np.finfo(np.float32).max
MIN_NORMAL = f(2.0 ** -126)
MIN_DENORM = f(2.0 ** -149)
MAX_DENORM = np.nextafter(MIN_NORMAL, f(0))
DENORM = f(1.0e-40)
HALF_PI = f(np.pi / 2)             # = kHalfPi 0x1.921fb6p+0
N_TRANSCRIBED_RANDOM = 1000        # of the random fill, the first this many items also go through the scalar Python transcription

KEY_SPHERE, KEY_CORNELL, KEY_QUAD, KEY_TRI, KEY_MISS = 0 << 28, 1 << 28, 2 << 28, 4 << 28, 0x7FFFFFFF
MAT_LAMBERT, MAT_MIRROR, MAT_GLASS, MAT_PHONG = 2, 3, 4, 5

PHONG_POWERS = [0.0, 0.5, 1.0, 2.0, 3.0, 80.0, 1.0e4, 1.0e6]
IORS = [1.0, 1.0 + 2.0 ** -23, 1.33, 1.75, 2.4, 0.5]
XI = [f(0), f(2.0 ** -24), f(0.5), f(1 - 2.0 ** -24)]


def ulps(x, k):
    """x moved k units in the last place (k < 0: towards -inf)"""
    x = f(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, INF if k > 0 else -INF)
    return x


def around(x, steps=(0, 1, 2)):
    return [ulps(x, s) for k in steps for s in ((k, -k) if k else (0,))]


class Case:
    def __init__(self, label, edges, fill, params=None, pdesc=None, no_ref=None):
        edges = np.asarray(edges, np.float32); fill = np.asarray(fill, np.float32)
        if edges.ndim == 1: edges = edges.reshape(-1, 1)
        if fill.ndim == 1: fill = fill.reshape(-1, 1)
        self.label, self.n_edge = label, edges.shape[0]
        self.inp = np.ascontiguousarray(np.concatenate([edges, fill.reshape(-1, edges.shape[1])]))
        self.params, self.pdesc = params, pdesc
        self.no_ref = dict(no_ref or {})             # edge index -> reason

    @property
    def words(self):
        return self.inp.view(np.uint32)

    def n_transcribed(self):
        return min(self.inp.shape[0], self.n_edge + N_TRANSCRIBED_RANDOM)


def rng_for(name):
    return np.random.default_rng([SEED] + [ord(c) for c in name])


def grid24(rng, n, lo=0):
    """n uniforms on the RNG's 2^-24 grid (art_math.h u01), in [lo * 2^-24, 1)"""
    return (rng.integers(lo, 1 << 24, n).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def units(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def positive_bits(rng, n, lo=1, hi=0x7F7FFFFF):
    """uniform over the positive binary32 bit patterns: denormals to FLT_MAX, every exponent equally likely"""
    return rng.integers(lo, hi + 1, n).astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------ math
def sincos_edges():
    e = []
    for k in range(-8, 9):
        e += around(f(k * np.pi / 2))                                   # k * pi/2 +- {0, 1, 2} ulp
    for m in range(-9, 9):
        e += around(f((m + 0.5) * np.pi / 2))                           # where v +- 0.5 changes k (art_math.h m1::sincos)
    e += [f(0.0), f(-0.0), MIN_NORMAL, -MIN_NORMAL, MIN_DENORM, -MIN_DENORM, MAX_DENORM, DENORM, -DENORM,
          ulps(2.0 ** 20, -1), -ulps(2.0 ** 20, -1), HALF_PI, -HALF_PI]
    return np.array(e, np.float32)


def sincos_case():
    rng = rng_for("sincos")
    e = sincos_edges()
    fill = np.concatenate([rng.uniform(-2 * np.pi, 2 * np.pi, 100000), 2.0 ** rng.uniform(-40, 20, 20000)]).astype(np.float32)
    fill = np.minimum(fill, ulps(2.0 ** 20, -1))
    # ART-M1 returns sin(-0) = +0 (r - (r z) q with r = -0), a libm returns -0; the renderer's angles are 2 pi xi >= +0, so no picture sees it
    no_ref = {int(i): "sin(-0): ART-M1 gives +0, the transcription's libm -0; never reached (angles are 2 pi xi)" for i in np.flatnonzero((e == 0) & np.signbit(e))}
    return Case("sincos", e, fill, no_ref=no_ref)


APOW_X = [f(0), DENORM, ulps(1, -1), f(1), ulps(1, 1), f(0.5), f(2), FLT_MAX, INF, f(-1), NAN]
APOW_Y = [f(0), DENORM, -DENORM] + around(0.5, (0, 1)) + around(1, (0, 1)) + around(2, (0, 1)) + \
         [f(-1), f(80), f(1e4), f(1e6), f(2) / f(81), f(1) / f(81), NAN]
# (x, y) with y * ln x next to +-200, the clamps of apow: y is the binary32 nearest to +-200 / ln x (mpmath, 200 bits); the list
# takes it and its two neighbours on either side, which puts (double)y * ln x on both sides of the clamp, 5e-6 .. 5e-5 away
APOW_CLAMP = [("0x1.000000p+1", "0x1.2089fcp+8"), ("0x1.000000p-1", "0x1.2089fcp+8"), ("0x1.400000p+3", "0x1.5b6f82p+6"),
              ("0x1.99999ap-4", "0x1.5b6f82p+6"), ("0x1.800000p+0", "0x1.ed42bcp+8"), ("0x1.800000p-1", "0x1.5b9b20p+9"),
              ("0x1.89374cp-9", "0x1.136d8ap+5"), ("0x1.f40000p+9", "0x1.cf3f58p+4")]


def apow_ys():
    """the exponents the scenes' Phong lobes produce: n, 2 / (n + 1), 1 / (n + 1)"""
    ys = []
    for n in PHONG_POWERS:
        ys += [f(n), f(2) / (f(n) + f(1)), f(1) / (f(n) + f(1))]
    return np.array(ys, np.float32)


def apow_case():
    rng = rng_for("apow")
    e = [(x, y) for x in APOW_X for y in APOW_Y]
    for xs, ys in APOW_CLAMP:
        x, y = f(float.fromhex(xs)), f(float.fromhex(ys))
        for s in (1, -1):
            e += [(x, ulps(s * y, k)) for k in (-2, -1, 0, 1, 2)]
    e = np.array(e, np.float32)
    no_ref = {}
    for i, (x, y) in enumerate(e):
        if np.isnan(x) or np.isnan(y): no_ref[i] = "NaN operand: Ada has no NaN literal, apow propagates it"
        elif x < 0: no_ref[i] = "negative base: Argument_Error in Ada, qNaN here"
        elif x == 0 and y <= 0: no_ref[i] = "0 ** (y <= 0): Argument_Error / Constraint_Error in Ada"
    ys = apow_ys()
    fill = np.stack([grid24(rng, 100000, 1), ys[rng.integers(0, len(ys), 100000)]], axis=1)
    fill[:64, 0] = f(1)                                                  # x = 1 of (0, 1]: the grid's own end point
    return Case("apow", e, fill, no_ref=no_ref)


SQRT_EDGES = [f(0), f(-0.0), MIN_DENORM, DENORM, MAX_DENORM, MIN_NORMAL, ulps(MIN_NORMAL, 1), FLT_MAX, ulps(FLT_MAX, -1), INF, f(-1), NAN] + \
             [v for sq in (4.0, 9.0, 2.25, 16769025.0, 2.0 ** -126 * 4, 2.0 ** 126, 2.0 ** -148) for v in around(sq, (0, 1))]
RCP_EDGES = [f(0), f(-0.0), MIN_DENORM, -MIN_DENORM, DENORM, MAX_DENORM, MIN_NORMAL, f(2.0 ** -127), f(2.0 ** 126), ulps(2.0 ** 126, 1), f(2.0 ** 127),
             FLT_MAX, -FLT_MAX, INF, -INF, NAN, f(3), f(1), ulps(1, 1), ulps(1, -1), f(1e-20), f(1e-25), f(1e-30), f(1e30)]


def sqrt_case():
    rng = rng_for("sqrt")
    return Case("sqrt", np.array(SQRT_EDGES, np.float32), positive_bits(rng, 50000))


def rcp_case():
    rng = rng_for("rcp")
    v = positive_bits(rng, 50000)
    return Case("rcp", np.array(RCP_EDGES, np.float32), np.where(rng.random(50000) < 0.5, v, -v))


def div_case():
    rng = rng_for("div")
    e = [(x, y) for x in RCP_EDGES for y in RCP_EDGES]
    a, b = positive_bits(rng, 50000), positive_bits(rng, 50000)
    near = rng.uniform(0.5, 2.0, 25000).astype(np.float32)
    a[:25000] = near; b[:25000] = rng.uniform(0.5, 2.0, 25000).astype(np.float32)      # half of them with quotients near 1: the rounding cases
    return Case("div", np.array(e, np.float32), np.stack([a, b], axis=1))


AXES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]
NEAR_AXES = [(1, 1e-5, 0), (1, float(ulps(1e-5, 1)), 0), (1e-5, 1, 1e-5), (0, 1, 2e-5), (1, 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (0.6, 0.8, 0), (1e-3, 1, -1e-3)]


def vec_edges():
    e = [(0, 0, 0), (1e-30, 0, 0), (1e-30, 1e-30, 1e-30), (1e-20, 1e-21, 0), (1e-23, 1e-23, 1e-23), (float(DENORM), 0, 0), (float(MIN_DENORM),) * 3,
         (1e19, 1e19, 1e19), (2e19, 0, 0), (float(FLT_MAX), 0, 0), (1e38, 1e38, 0), (3, 4, 0), (float(np.inf), 0, 0)]
    return np.array(e + AXES + NEAR_AXES, np.float32)


def normalize_case():
    rng = rng_for("normalize")
    v = rng.normal(size=(50000, 3)) * 10.0 ** rng.uniform(-24, 20, (50000, 1))
    return Case("normalize", vec_edges(), v.astype(np.float32))


def perpendicular_case():
    rng = rng_for("perpendicular")
    u = units(rng, 50000)
    u[:10000, rng.integers(0, 3)] *= f(1e-5)
    return Case("perpendicular", vec_edges(), u)


def reflect_case():
    rng = rng_for("reflect")
    e = []
    for n in AXES + NEAR_AXES[:4]:
        nn = np.array(ada.normalize(tuple(f(c) for c in n)), np.float32)
        e.append(np.concatenate([-nn, nn])); e.append(np.concatenate([nn, nn]))
        e.append(np.concatenate([np.roll(nn, 1), nn]))                  # d perpendicular to an axis n, exactly
        e.append(np.concatenate([np.zeros(3, np.float32), nn]))
    d, n = units(rng, 50000), units(rng, 50000)
    return Case("reflect", np.array(e, np.float32), np.concatenate([d, n], axis=1))


def log_pos_case():
    rng = rng_for("log_pos")
    sqrt2 = f(float.fromhex("0x1.6a09e6p+0"))
    e = around(1, (0, 1, 2)) + around(sqrt2, (0, 1, 2)) + around(sqrt2 / f(2), (0, 1)) + [f(0.5), f(2), MIN_DENORM, DENORM, MAX_DENORM, MIN_NORMAL, FLT_MAX, f(1e-30), f(1e30), f(np.e)]
    return Case("log_pos", np.array(e, np.float32), np.concatenate([positive_bits(rng, 50000), grid24(rng, 50000, 1)]))


def exp_small_case():
    rng = rng_for("exp_small")
    e = [f(0), f(-0.0), f(200), f(-200), ulps(200, -1), -ulps(200, -1), DENORM, -DENORM, MIN_DENORM, f(1e-10), f(-1e-10), f(1), f(-1), f(-87.3), f(-103.0), f(-103.9), f(88.7)]
    for m in range(-5, 6):
        e += around(f((m + 0.5) * np.log(2)), (0, 1))                   # where v +- 0.5 changes k (art_math.h m1::exp_small)
    fill = np.concatenate([rng.uniform(-200, 200, 100000), 2.0 ** rng.uniform(-40, 7, 20000) * rng.choice([-1.0, 1.0], 20000)]).astype(np.float32)
    return Case("exp_small", np.array(e, np.float32), np.clip(fill, -200, 200))


# ------------------------------------------------------------------------------------------------ sampling
def crit_cos(ior):
    """cosine of the critical angle on the dense side of an interface of index ior (ior < 1: the outside is the dense side)"""
    s = 1.0 / ior if ior > 1 else ior
    return f(np.sqrt(1.0 - s * s))


def geometry_edges(iors=()):
    """(d, n) pairs: incidence along -n exactly, d perpendicular to n exactly, cos = +-1e-7, rays from inside, axis-aligned and near-axis
    normals (the branches of perpendicular), and -- for glass -- cos at the critical angle +- {0, 1, 4} ulp, from both sides"""
    g = []
    for n in AXES[:3] + [AXES[4]] + NEAR_AXES[:2] + NEAR_AXES[8:]:
        nn = np.array(ada.normalize(tuple(f(c) for c in n)), np.float32)
        g += [(-nn, nn), (nn, nn)]
    y = np.array([0, 1, 0], np.float32)
    g += [(np.array([1, 0, 0], np.float32), y), (np.array([0, 0, -1], np.float32), y)]
    cs = [f(1e-7), f(-1e-7), f(0.5), f(-0.5), f(0.999), f(-0.999)]
    for ior in iors:
        if ior != 1.0:
            cs += [s * c for c in around(crit_cos(ior), (0, 1, 4)) for s in (f(1), f(-1))]
    for c in cs:
        g.append((np.array([np.sqrt(f(1) - c * c), c, 0], np.float32), y))           # dot(d, n) = c exactly
    return g


def random_dn(rng, n):
    d, nn = units(rng, n), units(rng, n)
    flip = (np.einsum("ij,ij->i", d, nn) > 0) & (rng.random(n) < 0.7)                 # most rays arrive from outside, the rest from inside
    d[flip] *= f(-1)
    graze = rng.random(n) < 0.05
    t = np.cross(nn, units(rng, n)); t /= np.linalg.norm(t, axis=1, keepdims=True)
    d[graze] = (t + nn * rng.uniform(-2e-3, 2e-3, (n, 1)))[graze].astype(np.float32)
    return d.astype(np.float32), nn


def material(mtype, p):
    p = [float(f(v)) for v in p] + [0.0] * (8 - len(p))
    return struct.pack("<ii8f", mtype, 0, *p)


def material_sets():
    """(label, type, parameters): Phong power, ior and albedo swept, not fixed"""
    out = [("lambert", MAT_LAMBERT, [0.25, 0.5, 0.0]), ("lambert_black", MAT_LAMBERT, [0, 0, 0]), ("lambert_white", MAT_LAMBERT, [1, 1, 1]),
           ("mirror", MAT_MIRROR, [0.75, 0.75, 0.75]), ("mirror_black", MAT_MIRROR, [0, 0, 0]), ("mirror_white", MAT_MIRROR, [1, 1, 1])]
    for ior in IORS:
        out.append(("glass_ior%.9g" % f(ior), MAT_GLASS, [0.75, 0.75, 0.75, 0.85, 0.85, 0.85, ior]))
    out += [("glass_black", MAT_GLASS, [0, 0, 0, 0, 0, 0, 1.75]), ("glass_white", MAT_GLASS, [1, 1, 1, 1, 1, 1, 1.75]), ("glass_opaque", MAT_GLASS, [1, 1, 1, 0, 0, 0, 1.75])]
    for pw in PHONG_POWERS:
        out.append(("phong_%g" % pw, MAT_PHONG, [0.75, 0.75, 0.75, pw]))
    out += [("phong_black", MAT_PHONG, [0, 0, 0, 80.0]), ("phong_white", MAT_PHONG, [1, 1, 1, 3.0])]
    return out


CANONICAL = {"lambert", "mirror", "glass_ior1.75", "phong_80"}        # the scene's own materials: the full random fill


def bsdf_sample_cases():
    cases = []
    for label, mtype, p in material_sets():
        rng = rng_for("bsdf_sample" + label)
        geo = geometry_edges([p[6]] if mtype == MAT_GLASS else ())
        e = [np.concatenate([[x1, x2], d, n]) for (d, n) in geo for x1 in XI for x2 in (XI if mtype in (MAT_LAMBERT, MAT_PHONG) else XI[:1])]
        n = 20000 if label in CANONICAL else 2000
        d, nn = random_dn(rng, n)
        fill = np.concatenate([grid24(rng, n)[:, None], grid24(rng, n)[:, None], d, nn], axis=1)
        cases.append(Case(label, np.array(e, np.float32), fill, params=material(mtype, p), pdesc=dict(type=mtype, p=[f(v) for v in p])))
    return cases


def bsdf_eval_cases():
    cases = []
    for label, mtype, p in material_sets():
        if mtype in (MAT_MIRROR, MAT_GLASS) and label not in CANONICAL:
            continue                                                     # no direct sampling of specular materials: one set each
        rng = rng_for("bsdf_eval" + label)
        e = []
        for (d, n) in geometry_edges():
            v = -d
            for l in (n, -n, v, np.array(ada.reflect(tuple(d), tuple(n)), np.float32), np.array([1, 0, 0], np.float32), np.array([np.sqrt(f(1) - f(1e-14)), 1e-7, 0], np.float32)):
                e.append(np.concatenate([l, v, n]))
        n = 20000 if label in CANONICAL else 2000
        d, nn = random_dn(rng, n)
        l = units(rng, n)
        spec = np.array([ada.reflect(tuple(a), tuple(b)) for a, b in zip(d[:200], nn[:200])], np.float32)
        l[:200] = spec                                                   # l at the lobe's axis: ct = 1 -+ a few ulp, apow's x == 1 case
        fill = np.concatenate([l, -d, nn], axis=1)
        cases.append(Case(label, np.array(e, np.float32), fill, params=material(mtype, p), pdesc=dict(type=mtype, p=[f(v) for v in p])))
    return cases


def sample_cosine_case(name):
    rng = rng_for(name)
    e = []
    for (d, n) in geometry_edges():
        for pw in PHONG_POWERS:
            for x1 in XI:
                for x2 in XI:
                    e.append(np.concatenate([[x1, x2], -d if np.dot(d, n) < 0 else d, n, [pw]]))      # direction: a reflected ray, on n's side
    n = 20000
    d, nn = random_dn(rng, n)
    pw = np.array(PHONG_POWERS, np.float32)[rng.integers(0, len(PHONG_POWERS), n)]
    lam = rng.random(n) < 0.3
    d[lam] = nn[lam]; pw[lam] = 1                                       # Lambert's call: direction = normal, power 1
    fill = np.concatenate([grid24(rng, n)[:, None], grid24(rng, n)[:, None], -d, nn, pw[:, None]], axis=1)
    return Case(name, np.array(e, np.float32), fill)


def fresnel_case():
    rng = rng_for("fresnel")
    e = []
    for ior in IORS:
        cs = [f(1), f(-1), f(0), f(-0.0), f(1e-7), f(-1e-7), f(0.5), f(-0.5)]
        if ior != 1.0:
            cs += [s * c for c in around(crit_cos(ior), (0, 1, 4)) for s in (f(1), f(-1))]
        e += [(c, f(ior), f(1)) for c in cs]
    n = 20000
    fill = np.stack([rng.uniform(-1, 1, n), np.array(IORS)[rng.integers(0, len(IORS), n)], np.ones(n)], axis=1)
    return Case("fresnel", np.array(e, np.float32), fill.astype(np.float32))


def light(d):
    return struct.pack("<ii9f3ff3ff", d["shape"], 4, *[float(v) for k in ("boxMin", "boxMax", "normal") for v in d[k]], *[float(v) for v in d["center"]],
                       float(d["radius"]), *[float(v) for v in d["intensity"]], float(d["surfaceArea"]))


V = ada.V
SPHERE_LIGHT = dict(shape=1, boxMin=V(0, 0, 0), boxMax=V(0, 0, 0), normal=V(0, -1, 0), center=V(0.0, 4.5, 1.0), radius=f(0.5),
                    intensity=V(10, 10, 10), surfaceArea=f(f(4.0) * f(np.pi) * f(0.5) * f(0.5)))                          # scene.adb:104-122
RECT_LIGHT = dict(shape=0, boxMin=V(-0.75, 4.98, 1.25), boxMax=V(0.75, 4.98, 3.25), normal=V(0, -1, 0), center=V(0, 0, 0), radius=f(0),
                  intensity=V(20, 20, 20), surfaceArea=f(f(1.5) * f(2.0)))
LIGHTS = [("sphere_light", SPHERE_LIGHT), ("rect_light", RECT_LIGHT)]


def light_points(L, rng, n):
    c, r = np.array(L["center"], np.float32), L["radius"]
    e = []
    if L["shape"] == 1:
        for a in AXES:
            a = np.array(a, np.float32)
            e += [c + r * a, c + ulps(r, -8) * a, c + ulps(r, 8) * a, c + f(0.25) * a, c + f(0.51) * a, c + f(1e6) * a, c + f(1e-3) * a]     # on the surface, just inside / outside, far
        e += [c, c + np.array([0.3, -0.4, 0], np.float32), np.array([0, 0, 0], np.float32), np.array([1e6, 1e6, 1e6], np.float32)]
    else:
        y = L["boxMin"][1]
        for x, z in ((0, 2.25), (-0.75, 1.25), (0.75, 3.25), (2.0, 0.5), (0.3, 2.0)):
            e += [np.array([x, yy, z], np.float32) for yy in (y, ulps(y, -1), ulps(y, 1), f(5.0), f(4.0), f(0.0), y - f(1e-20), f(1e6), f(-1e6))]      # in, below, above the light's plane
    pts = rng.random((n, 3)) * [5.0, 4.99, 5.0] + [-2.5, 0.0, 0.0]
    if L["shape"] == 1:
        k = n // 20
        pts[:k] = c + units(rng, k) * rng.uniform(0, 0.6, (k, 1))      # in and around the light sphere: the uniform-sphere branch
    return np.array(e, np.float32), pts.astype(np.float32)


def light_cases(op):
    cases = []
    for label, L in LIGHTS:
        if op == "sphere_light_pdf" and L["shape"] != 1:
            continue
        rng = rng_for(op + label)
        pe, pr = light_points(L, rng, 20000)
        if op == "light_sample":
            e = [np.concatenate([[a, b], p]) for p in pe for a in XI for b in XI]
            fill = np.concatenate([grid24(rng, 20000)[:, None], grid24(rng, 20000)[:, None], pr], axis=1)
        elif op == "light_eval_pdf":
            dirs = [np.array(a, np.float32) for a in AXES] + [np.array([1e-7, np.sqrt(f(1) - f(1e-14)), 0], np.float32), np.array([0.6, 0.8, 0], np.float32)]
            e = [np.concatenate([p, d, [t]]) for p in pe for d in dirs for t in (f(0), f(1e-20), f(1), f(1e6), f(1e19), f(1e20))]
            fill = np.concatenate([pr, units(rng, 20000), rng.uniform(0.1, 6.1, (20000, 1)).astype(np.float32)], axis=1)
        else:
            e, fill = pe, pr
        cases.append(Case(label, np.array(e, np.float32), fill, params=light(L), pdesc=L))
    return cases


def pdf_area_case():
    rng = rng_for("pdf_area_to_solid")
    cs = [f(0), f(-0.0), f(-1), f(1), f(1e-21)] + around(1e-20, (0, 1)) + [DENORM, f(1e-7), NAN]
    e = [(a, d, c) for a in (f(1) / f(3), f(0), f(1e30)) for d in (f(0), f(1e-20), DENORM, f(1), f(1e6), f(1e19), f(1e20)) for c in cs]
    fill = np.stack([rng.uniform(0.01, 10, 20000), rng.uniform(0, 10, 20000), rng.uniform(-0.2, 1, 20000)], axis=1)
    return Case("pdf_area_to_solid", np.array(e, np.float32), fill.astype(np.float32))


# ------------------------------------------------------------------------------------------------ hits
def tri_case():
    rng = rng_for("tri_raw")
    e = []
    down = [0, 0, -1]
    # det = e1 . cross(d, e2) = a for B = (a, 0, 0), C = (0, 1, 0), d = (0, 0, -1): det at the 1e-25 clamp +- 1 ulp, 0, -tiny, a denormal
    for a in around(1e-25, (0, 1)) + [f(0), f(-1e-30), -DENORM, DENORM, f(-1), f(1e-24), f(1e-26)]:
        for ox in (f(0.25) * a, f(0.25)):
            e.append(np.concatenate([[ox, 0.25, 1], down, [0, 0, 0], [a, 0, 0], [0, 1, 0]]))
    # A = 0, B = x, C = y, d = -z, o = (x, y, 1): u = y, v = x, t = 1 -- on an edge, on a vertex, u + v = 1 -+ 1 ulp
    h = f(0.5)
    for x, y in [(0, 0.5), (0.5, 0), (0.5, 0.5), (h, ulps(h, -1)), (h, ulps(h, 2)), (ulps(h, -1), h), (0, 0), (1, 0), (0, 1), (float(MIN_DENORM), 0.5), (0.5, float(MIN_DENORM)),
                 (-float(MIN_DENORM), 0.5), (0.5, -float(MIN_DENORM)), (0.25, 0.25), (0.7, 0.7), (-0.1, 0.5), (0.5, -0.1), (float(ulps(1, -1)), float(MIN_DENORM))]:
        for oz in (1, 0, -1):                                            # in front, origin on the plane, behind
            e.append(np.concatenate([[x, y, oz], down, [0, 0, 0], [1, 0, 0], [0, 1, 0]]))
    for tri in ([0, 0, 0] * 3, [0, 0, 0, 1, 0, 0, 2, 0, 0], [1, 1, 1, 1, 1, 1, 0, 1, 0], [0, 0, 0, 1, 0, 0, 1, 0, 0]):      # degenerate triangles
        e.append(np.concatenate([[0.25, 0.25, 1], down, tri]))
        e.append(np.concatenate([[0.25, 0.25, 1], [0, 0, 0], tri]))
    e.append(np.concatenate([[0.25, 0.25, 1], [1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]]))                                # ray in the plane's direction
    n = 50000
    A = rng.uniform(-2, 2, (n, 3)); B = A + rng.normal(size=(n, 3)) * 0.5; C = A + rng.normal(size=(n, 3)) * 0.5
    uv = rng.uniform(-0.3, 1.0, (n, 2))
    uv[: n // 5] = np.round(uv[: n // 5] * 4) / 4                       # a fifth aimed exactly at edge points and vertices (as far as rounding lets them)
    tgt = A + (B - A) * uv[:, :1] + (C - A) * uv[:, 1:]
    o = rng.uniform(-3, 3, (n, 3))
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    flip = rng.random(n) < 0.5
    B[flip], C[flip] = C[flip].copy(), B[flip].copy()                   # both windings: the one-sided test rejects half of them
    return Case("tri_raw", np.array(e, np.float32), np.concatenate([o, d, A, B, C], axis=1).astype(np.float32))


def sphere_case():
    rng = rng_for("sphere")
    z = [0, 0, 1]
    e = [np.concatenate([[0, 0, -5], z, [0, 1, 0, 1]]),                 # disc = 0: the tangent ray
         np.concatenate([[0, 0, -5], z, [0, float(ulps(1, 1)), 0, 1]]), np.concatenate([[0, 0, -5], z, [0, float(ulps(1, -1)), 0, 1]]),
         np.concatenate([[0, 0, -1], z, [0, 0, 0, 1]]),                 # origin on the surface, looking in and out
         np.concatenate([[0, 0, 1], z, [0, 0, 0, 1]]), np.concatenate([[0, 0, 0], z, [0, 0, 0, 1]]), np.concatenate([[0.3, 0.2, 0.1], z, [0, 0, 0, 1]]),
         np.concatenate([[0, 0, 5], z, [0, 0, 0, 1]]), np.concatenate([[0, 0, -5], z, [0, 0, 0, 0]]), np.concatenate([[0, 0, -5], [0, 0, 0], [0, 0, 0, 1]]),
         np.concatenate([[0, 0, -1e20], z, [0, 0, 0, 1]]), np.concatenate([[0, 0, -3e19], z, [0, 0, 0, 1e19]]), np.concatenate([[0, 0, -5], z, [0, 0, 0, float(DENORM)]])]
    n = 50000
    c = rng.uniform(-2, 2, (n, 3)); r = rng.uniform(0.1, 1.5, (n, 1))
    o = c + units(rng, n) * r * rng.uniform(0, 4, (n, 1))               # origins inside (a quarter) and outside
    tgt = c + units(rng, n) * r * rng.uniform(0, 1.3, (n, 1))           # aimed through, at the rim and past it
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return Case("sphere", np.array(e, np.float32), np.concatenate([o, d, c, r], axis=1).astype(np.float32))


CORNELL = dict(min=V(-2.5, 0, 0), max=V(2.5, 5, 5), mat=(2, 3, 1, 1, 8, 1), nrm=(V(1, 0, 0), V(-1, 0, 0), V(0, 1, 0), V(0, -1, 0), V(0, 0, 1), V(0, 0, -1)))


def cornell_case():
    rng = rng_for("cornell")
    o0 = np.array([0, 2.5, 2.5], np.float32)
    e = []
    eps = f(1e-5)
    deltas = [f(0)] + around(eps, (0, 1)) + [f(0.5e-5), f(2e-5), f(9e-6)]
    # exit points within 1e-5 +- 1 ulp of two faces at once (the corner rule: the later face wins), every pair of adjacent faces
    for face, other in [((0, 2.5), (1, 5.0)), ((0, 2.5), (1, 0.0)), ((0, -2.5), (1, 5.0)), ((0, -2.5), (2, 0.0)), ((1, 5.0), (2, 0.0)), ((1, 0.0), (2, 0.0)),
                        ((0, 2.5), (2, 5.0)), ((1, 0.0), (2, 5.0)), ((0, -2.5), (1, 0.0))]:
        for dl in deltas:
            for oo in (o0, np.array([0.5, 1.0, 4.0], np.float32)):
                tgt = np.array([0.3, 2.0, 1.5], np.float64)
                tgt[face[0]] = face[1]
                tgt[other[0]] = other[1] - float(dl) * np.sign(other[1] - 2.0)
                d = tgt - oo; d /= np.linalg.norm(d)
                e.append(np.concatenate([oo, d.astype(np.float32)]))
    for a in AXES:                                                       # axis-parallel rays: 1 / 0 = inf, and the open face (+z)
        e.append(np.concatenate([o0, np.array(a, np.float32)]))
        e.append(np.concatenate([np.array([2.5, 5, 0], np.float32), np.array(a, np.float32)]))       # origin on three planes: 0 * inf
        e.append(np.concatenate([np.array([0, 2.5, -3], np.float32), np.array(a, np.float32)]))      # from outside
    e.append(np.concatenate([o0, [0, 0, 0]])); e.append(np.concatenate([o0, [-0.0, 1, -0.0]]))
    n = 50000
    o = rng.uniform([-2.5, 0, 0], [2.5, 5, 5], (n, 3)); o[: n // 10] = rng.uniform(-6, 9, (n // 10, 3))
    d = units(rng, n)
    d[n // 10: n // 5, rng.integers(0, 3)] = 0
    return Case("cornell", np.array(e, np.float32), np.concatenate([o, d], axis=1).astype(np.float32),
                params=struct.pack("<6f", *[float(v) for v in CORNELL["min"] + CORNELL["max"]]), pdesc=CORNELL)


def quad_case():
    rng = rng_for("quad")
    L = RECT_LIGHT
    e = []
    up = [0, 1, 0]
    for x in around(L["boxMin"][0], (0, 1)) + around(L["boxMax"][0], (0, 1)) + [f(0)]:
        for z in around(L["boxMin"][2], (0, 1)) + around(L["boxMax"][2], (0, 1)) + [f(2)]:
            e.append(np.concatenate([[x, 0, z], up]))                    # hp on the quad's border and one ulp either side
    for dy in (f(0), f(-0.0), DENORM, -DENORM, f(1e-30)):
        for oy in (f(1), L["boxMax"][1], f(5)):
            e.append(np.concatenate([[0, oy, 2], [0.6, dy, 0.8]])); e.append(np.concatenate([[0, oy, 2], [0, dy, 0]]))
    e += [np.concatenate([[0, 4.98, 2], up]), np.concatenate([[0, 5, 2], up]), np.concatenate([[0, 5, 2], [0, -1, 0]]), np.concatenate([[0, 4.98, 2], [0, -1, 0]])]
    n = 50000
    o = rng.uniform([-2.5, 0, 0], [2.5, 5.5, 5], (n, 3))
    tgt = np.stack([rng.uniform(-1.2, 1.2, n), np.full(n, 4.98), rng.uniform(0.8, 3.7, n)], axis=1)
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: n // 10] = units(rng, n // 10)
    # two fifths aimed AT the border lines: hp = o + t * d then lands within an ulp or two of the bound of a strict comparison, where a
    # fused o + t * d and the two roundings of the contract give different answers
    k = 2 * n // 5
    edge = tgt[n - k:].copy()
    side = rng.integers(0, 4, k)
    edge[:, 0] = np.where(side == 0, -0.75, np.where(side == 1, 0.75, rng.uniform(-0.75, 0.75, k)))
    edge[:, 2] = np.where(side == 2, 1.25, np.where(side == 3, 3.25, rng.uniform(1.25, 3.25, k)))
    o[n - k:, 1] = rng.uniform(0, 4.9, k)
    de = edge - o[n - k:]; d[n - k:] = de / np.linalg.norm(de, axis=1, keepdims=True)
    return Case("quad", np.array(e, np.float32), np.concatenate([o, d], axis=1).astype(np.float32), params=light(L), pdesc=L)


def slab_case():
    rng = rng_for("slab")
    lo, hi = [-1, -1, -1], [1, 2, 3]
    e = []
    small = [f(0), f(-0.0), f(1e-31), f(-1e-31), ulps(1e-30, -1), f(1e-30), DENORM]
    for s in small:
        for o in ([0, 0, -5], [-1, 0.5, -5], [1, 2, 3], [-1, -1, -1], [5, 0.5, 0.5], [0, 0, 0]):      # inside the slab, on a box plane, outside
            for tb in (FLT_MAX, f(4)):
                e.append(np.concatenate([o, [s, s, 1], lo, hi, [tb]])); e.append(np.concatenate([o, [1, s, -s], lo, hi, [tb]])); e.append(np.concatenate([o, [s, s, s], lo, hi, [tb]]))
    for o in ([1e30, 0, 0], [-1e30, 1e30, 0], [3e38, 3e38, 3e38], [1e10, 0, 0]):                       # o * inv overflows: plane * inv - o * inv = inf - inf without the fused form
        for d in ([1e-31, 0, 1], [1e-20, 1e-20, 1], [-0.0, 1e-31, 1]):
            e.append(np.concatenate([o, d, lo, hi, [FLT_MAX]])); e.append(np.concatenate([o, d, [-3e38, -1, -1], [3e38, 1, 1], [FLT_MAX]]))
    e.append(np.concatenate([[0, 0, -5], [0, 0, 1], [0, 0, 0], [0, 0, 0], [FLT_MAX]]))                 # a box that is a point
    e.append(np.concatenate([[0, 0, -5], [0, 0, 1], lo, hi, [0]])); e.append(np.concatenate([[0, 0, -5], [0, 0, 1], lo, hi, [4]])); e.append(np.concatenate([[0, 0, -5], [0, 0, 1], lo, hi, [float(ulps(4, -1))]]))
    n = 50000
    c = rng.uniform(-3, 3, (n, 3)); half = rng.uniform(0, 1.5, (n, 3))
    o = rng.uniform(-5, 5, (n, 3))
    o[: n // 10] = (c - half)[: n // 10] * [1, 0, 0] + o[: n // 10] * [0, 1, 1]                         # origin on a box plane
    tgt = c + half * rng.uniform(-1.4, 1.4, (n, 3))
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    z = rng.random((n, 3)) < 0.05
    d[z] = 0
    tb = np.where(rng.random(n) < 0.5, float(FLT_MAX), rng.uniform(0, 10, n))
    return Case("slab", np.array(e, np.float32), np.concatenate([o, d, c - half, c + half, tb[:, None]], axis=1).astype(np.float32))


def cand_wins_case():
    rng = rng_for("cand_wins")
    ts = np.array([f(0), f(-0.0), f(1), ulps(1, 1), ulps(1, -1), FLT_MAX, INF, NAN, f(-1), DENORM], np.float32)
    keys = np.array([0, 1, 5, KEY_CORNELL | 2, KEY_QUAD, KEY_TRI | 3, KEY_TRI | 4, KEY_MISS], np.uint32)
    e = np.array([(t.view(np.uint32), k, b.view(np.uint32), kb) for t in ts for k in keys for b in ts for kb in keys], np.uint32)
    n = 50000
    pool = np.concatenate([ts[:7], rng.uniform(0, 10, 9).astype(np.float32)])
    fill = np.stack([pool[rng.integers(0, len(pool), n)].view(np.uint32), keys[rng.integers(0, len(keys), n)],
                     pool[rng.integers(0, len(pool), n)].view(np.uint32), keys[rng.integers(0, len(keys), n)]], axis=1).astype(np.uint32)
    return Case("cand_wins", e.view(np.float32), fill.view(np.float32))


# ------------------------------------------------------------------------------------------------ the camera ray
CAMERA_FRAMES = [(1, 1), (1, 7), (7, 1), (2, 2), (67, 5), (5, 67), (257, 3), (4096, 2160)]
CAMERA_ALL_PIXELS = 257 * 3                        # frames up to this many pixels: every pixel is an edge item
CAMERA_FOVS = [0.01, np.pi / 6, 3.0]               # radians, next to the reference's pi / 2: from 0.57 to 172 degrees
REFERENCE_CAMERA = (0.0, 2.55, 12.5)               # = scenes.REFERENCE_CAMERA (scene.adb:212), asserted by tests/test_device_kat_host.py
ROTATIONS = [(0.3, (0, 1, 0)), (-1.1, (1, 2, 3)), (2.5, (-0.5, 0.1, 0.7))]      # (angle, axis) of the arbitrary rotations


def _ident():
    return [[f(1) if r == c else f(0) for c in range(4)] for r in range(4)]


def _quarter_turn(axis):
    """the exact quarter turn about axis 0 / 1 / 2: entries 0 and +-1, no cosine of a rounded pi / 2"""
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    m = _ident()
    m[a][a] = m[b][b] = f(0); m[a][b] = f(-1); m[b][a] = f(1)
    return m


def _translated(m, t):
    m = [row[:] for row in m]
    for r in range(3):
        m[r][3] = f(t[r])
    return m


def camera_matrices():
    out = [("identity", _ident()), ("reference_camera", _translated(_ident(), REFERENCE_CAMERA))]
    out += [("quarter_%s" % "xyz"[k], _quarter_turn(k)) for k in range(3)]
    rots = [("rot%d" % k, ada.rotation_matrix(f(a), V(*ax))) for k, (a, ax) in enumerate(ROTATIONS)]
    out += rots
    out += [(name + "_moved", _translated(m, t)) for (name, m), t in zip(rots, [REFERENCE_CAMERA, (-0.75, 0.1, 3.1), (0.25, -0.5, 0.125)])]
    return out


def camera_params(d):
    return struct.pack("<iiif16f", d["width"], d["height"], d["aa_on"], float(d["cam_z"]), *[float(v) for row in d["matrix"] for v in row])


def camera_pixels(W, H):
    """every pixel of a small frame; of a large one the corners, the centre pixel(s), the last pixel and the ends of the first two rows"""
    if W * H <= CAMERA_ALL_PIXELS:
        return list(range(W * H))
    xs = sorted({0, 1, (W - 1) // 2, W // 2, W - 2, W - 1}); ys = sorted({0, 1, (H - 1) // 2, H // 2, H - 2, H - 1})
    return [y * W + x for y in ys for x in xs]


def camera_cases():
    mats = camera_matrices()
    cases = []
    for W, H in CAMERA_FRAMES:
        zs = [("fov_ref", ada.eye_ray_z(W))] + [("fov_%g" % fov, ada.eye_ray_z(W, fov)) for fov in CAMERA_FOVS]
        combos = [(m, zs[0]) for m in mats] + [(m, z) for m in (mats[0], mats[-1]) for z in zs[1:]]
        for (mname, m), (zname, z) in combos:
            for aa in (1, 0):
                label = "%dx%d_%s_%s_%s" % (W, H, mname, zname, "aa" if aa else "noaa")
                rng = rng_for("camera_dir" + label)
                samples = range(8) if aa else (0, 5)                   # AA on: bit 2 must not matter; AA off: the sample must not matter
                e = np.array([(p, s) for p in camera_pixels(W, H) for s in samples], np.uint32)
                n = 2000 if W * H > CAMERA_ALL_PIXELS else 200
                fill = np.stack([rng.integers(0, W * H, n), rng.integers(0, 1 << 32, n)], axis=1).astype(np.uint32)
                d = dict(width=W, height=H, aa_on=aa, cam_z=z, matrix=m)
                cases.append(Case(label, e.view(np.float32), fill.view(np.float32), params=camera_params(d), pdesc=d))
    return cases


# ------------------------------------------------------------------------------------------------ the LDR frame
RESOLVE_SPPS = [1, 3, 4, 7, 256, 1 << 24]
TOP_FINITE_WORD = 0x7F7FFFFF


def _w2f(w):
    return np.uint32(w).view(np.float32)


def rise_word(byte_of, k):
    """the smallest positive binary32 word w with byte_of(w) > k, by bisection: byte_of is non-decreasing over the positive words (a
    product, a correctly rounded root, a minimum, a product and a rounding, each of them monotone)"""
    lo, hi = 0, TOP_FINITE_WORD                                          # byte_of(lo) <= k < byte_of(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if byte_of(mid) > k: hi = mid
        else: lo = mid
    return hi


def _rises(value_of):
    byte_of = lambda w: ada.to_unsigned_32(value_of(_w2f(w)))
    return [rise_word(byte_of, k) for k in range(255)]


# computed at import time from the transcription alone: per spp, for k = 0..254 the accumulated sum (as a word) at which the byte rises
# from k to k + 1; and the same for the value s = after the gamma, of which min(s, 1) * 255 is converted
RESOLVE_RISES = {spp: _rises(lambda a, n=f(1) / f(spp): ada.resolve_channel(a, n)) for spp in RESOLVE_SPPS}
ROUND_RISES = _rises(lambda s: ada.amin(s, f(1)) * f(255))

RESOLVE_SPECIALS = [f(0), f(-0.0), MIN_DENORM, DENORM, MAX_DENORM, MIN_NORMAL, -MIN_DENORM, -DENORM, f(-1e-30), f(-1), -FLT_MAX, NAN, INF, -INF,
                    f(1e-30), f(1e-10), f(0.25), f(0.5), f(2), f(1e3), f(1e6), f(1e30), FLT_MAX]


def resolve_case():
    rng = rng_for("resolve")
    e = []
    for spp in RESOLVE_SPPS:
        norm = f(1) / f(spp)
        sp = RESOLVE_SPECIALS + around(f(spp), (0, 1, 2))               # the last five: 1.0 after the gamma and one, two ulp either side
        for i in range(len(sp)):                                         # every special in every channel, next to two others
            e.append((sp[i], sp[(i + 1) % len(sp)], sp[(i + 7) % len(sp)], norm))
        e += [(f(0), f(-0.0), MIN_DENORM, norm), (FLT_MAX, INF, f(spp), norm)]      # black and white
        rises = RESOLVE_RISES[spp]
        for k in range(255):
            for step in (-1, 0, 1):                                      # below the rise, at it, above it; green and blue at other bytes' rises
                e.append((_w2f(rises[k] + step), _w2f(rises[(k + 85) % 255] + step), _w2f(rises[(k + 170) % 255] + step), norm))
    # 150 000 random items: the boundary items above sit on ties by construction, where binary32 and float64 may round to different bytes;
    # the random fill keeps them a small share of the set (tests/test_device_kat_host.py caps the one-off items at 2 % of all items)
    n = 150000
    spp = np.array(RESOLVE_SPPS)[rng.integers(0, len(RESOLVE_SPPS), n)]
    acc = (rng.uniform(0, 1.2, (n, 3)) ** 2 * spp[:, None]).astype(np.float32)        # bytes spread evenly, a sixth of them clamped
    acc[: n // 10] = positive_bits(rng, 3 * (n // 10)).reshape(-1, 3)
    fill = np.concatenate([acc, (f(1) / spp.astype(np.float32))[:, None]], axis=1)
    e = np.array(e, np.float32)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(e[:, :3]) | (e[:, :3] < 0)
    no_ref = {int(i): "a negative or NaN sum: \"**\" raises Argument_Error in the Ada text; the oracle and the host build hold it" for i in np.flatnonzero(bad.any(axis=1))}
    return Case("resolve", e, fill, no_ref=no_ref)


ROUND_TOP = _w2f(0x4F7FFFFF)                        # the largest binary32 below 2^32: above it a uint32_t conversion is undefined in C++
ROUND_SPECIALS = [f(0), f(-0.0), MIN_DENORM, DENORM, MIN_NORMAL, -MIN_DENORM, f(-0.25), f(-0.5), f(-1), -FLT_MAX, -INF, NAN, f(1), f(255), ulps(255, 1), f(255.5), f(256),
                  f(1e6), f(8388607.5), f(8388608), f(16777215), f(16777216), f(2.0 ** 31), ulps(2.0 ** 31, -1), ROUND_TOP]


def round_u32_case():
    """resolve_pixel hands ada_round_u32 values of [0, 255] only; the list goes on to the end of the function's domain"""
    rng = rng_for("round_u32")
    e = list(ROUND_SPECIALS)
    for k in range(255):
        e += [ada.amin(_w2f(ROUND_RISES[k] + step), f(1)) * f(255) for step in (-1, 0, 1)]      # what the resolve converts around the rise of s
        e += around(f(k) + f(0.5), (0, 1))                                                         # the tie itself: exactly k + 0.5, and its neighbours
    n = 50000
    fill = rng.uniform(0, 256, n).astype(np.float32)
    fill[: n // 10] = positive_bits(rng, n // 10, hi=0x4F7FFFFF)
    fill[n // 10: n // 5] *= f(-1)
    e = np.array(e, np.float32)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(e) | (e <= f(-0.5))
    no_ref = {int(i): "NaN or below -0.5: no NaN literal / Constraint_Error in Ada; the product's rule (0) is held by the host build" for i in np.flatnonzero(bad)}
    return Case("round_u32", e, fill, no_ref=no_ref)


def colour_lum_case():
    rng = rng_for("colour_lum")
    sp = [f(0), f(-0.0), MIN_DENORM, DENORM, MIN_NORMAL, f(1), f(-1), f(1) / f(3), f(0.5), f(1e-20), f(1e20), FLT_MAX, -FLT_MAX, INF, -INF, NAN]
    e = [(a, b, c) for a in sp for b in sp for c in sp]
    n = 50000
    fill = rng.uniform(0, 20, (n, 3)).astype(np.float32)
    fill[: n // 10] = positive_bits(rng, 3 * (n // 10)).reshape(-1, 3)
    fill[n // 10: n // 5] *= rng.choice([-1.0, 1.0], (n // 10, 3)).astype(np.float32)
    return Case("colour_lum", np.array(e, np.float32), fill)


_BUILDERS = {
    "camera_dir": camera_cases, "resolve": lambda: [resolve_case()], "round_u32": lambda: [round_u32_case()], "colour_lum": lambda: [colour_lum_case()],
    "sincos": lambda: [sincos_case()], "tan": lambda: [sincos_case()], "sincos_f64": lambda: [sincos_case()], "apow": lambda: [apow_case()], "sqrt": lambda: [sqrt_case()], "rcp": lambda: [rcp_case()],
    "div": lambda: [div_case()], "normalize": lambda: [normalize_case()], "reflect": lambda: [reflect_case()], "perpendicular": lambda: [perpendicular_case()],
    "log_pos": lambda: [log_pos_case()], "exp_small": lambda: [exp_small_case()],
    "sample_cosine": lambda: [sample_cosine_case("sample_cosine")], "sample_cosine_fixed": lambda: [sample_cosine_case("sample_cosine_fixed")],
    "fresnel": lambda: [fresnel_case()], "light_sample": lambda: light_cases("light_sample"), "light_eval_pdf": lambda: light_cases("light_eval_pdf"),
    "sphere_light_pdf": lambda: light_cases("sphere_light_pdf"), "pdf_area_to_solid": lambda: [pdf_area_case()],
    "bsdf_sample": bsdf_sample_cases, "bsdf_eval": bsdf_eval_cases,
    "tri_raw": lambda: [tri_case()], "sphere": lambda: [sphere_case()], "cornell": lambda: [cornell_case()], "quad": lambda: [quad_case()], "slab": lambda: [slab_case()],
    "cand_wins": lambda: [cand_wins_case()],
}
_cache = {}


def cases(op):
    """the Cases of op, built once per process"""
    if op not in _cache:
        _cache[op] = _BUILDERS[op]()
    return _cache[op]
