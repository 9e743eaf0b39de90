"""The device-resident ray queries (art_trace_rays_device / art_occluded_rays_device) as a rule in numpy binary32, written from the
sentences of include/art_hip.h, csrc/art_query.h and the header comment of csrc/art_query.hip -- not from anything the product returns.

Inputs: the caller's o, d [n, 3], optional tnear, tfar [n], and the closest hits an independent scan found for the SHIFTED rays
(shifted() gives those rays; tests/orc.py closest_hits is the scan the GPU tests use, the host tests plant the hits).

  t0 = tnear > 0 ? tnear : 0                (tnear NULL: 0, and the origin is left as it is)
  o' = o + t0 * d                           one binary32 multiply, one binary32 add, per component
  f  = tfar - t0                            (tfar NULL: Float'Last, "the bound art_trace_rays uses")
  live = f > 0                              (!(tfar - t0 > 0) is an empty interval: a miss)
  hit  = live and the scan hits o' + t' d with t' < f          (strict: a hit AT the bound is beyond it)
  a hit:  t = fl32(t0 + t'), is_hit 1, prim_type, prim_index, mat_id, mat, normal, u, v those of the scan
  a miss: t = f ("a miss holds t = the bound"), is_hit 0, the four id words -1, normal = 0, u = v = 0
  occluded = hit

A record is the 11 words of ArtHit: t | is_hit | prim_type | prim_index | mat_id | mat | normal[3] | u | v.  The scan's records have
the same first nine words (tests/orc.py Hit); its last two are texture coordinates, which ArtHit does not carry: u, v are the
triangle's barycentrics, "weight of C, weight of B" (geometry.adb:231-263), which barycentrics() computes for the triangle the scan names,
and 0 for every other primitive."""
import numpy as np

F = np.float32
NO_BOUND = F(3.4028234663852886e38)      # Float'Last: what a NULL tfar stands for
WORDS = 11
T, IS_HIT, PRIM_TYPE, PRIM_INDEX, MAT_ID, MAT, NX, NY, NZ, U, V = range(WORDS)
PRIM_TRIANGLE = 2                          # Primitive'Pos: 0 plane, 1 sphere, 2 triangle, 3 quad


def _f(a):
    return None if a is None else np.ascontiguousarray(a, F)


def shifted(o, d, tnear=None, tfar=None):
    """-> (o' [n, 3], f [n], t0 [n], live [n]): the ray that is traced, its bound, the shift and whether the interval holds anything"""
    o, d, tnear, tfar = _f(o), _f(d), _f(tnear), _f(tfar)
    n = o.shape[0]
    if tnear is None:
        t0, os_ = np.zeros(n, F), o.copy()                                   # no shift without tnear
    else:
        t0 = np.where(tnear > 0, tnear, F(0)).astype(F)
        with np.errstate(over="ignore", invalid="ignore"):
            prod = (t0[:, None] * d).astype(F)                               # the multiply, rounded ...
            os_ = (o + prod).astype(F)                                       # ... then the add
    bound = np.full(n, NO_BOUND, F) if tfar is None else tfar
    with np.errstate(over="ignore", invalid="ignore"):
        f = (bound - t0).astype(F)
    return os_, f, t0, f > 0


def barycentrics(o, d, A, B, C):
    """IntersectTriangle's t, u, v (geometry.adb:231-263) of rays o + t d against triangles A, B, C, all [n, 3], in binary32 in the
    order the text writes them; u weights C, v weights B.  No acceptance test: the caller names the triangle that was hit."""
    o, d, A, B, C = (np.asarray(x, F) for x in (o, d, A, B, C))

    def sub(a, b):
        return a - b

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)

    with np.errstate(all="ignore"):
        e1, e2 = sub(B, A), sub(C, A)
        pv = cross(d, e2)
        tv = sub(o, A)
        qv = cross(tv, e1)
        det = dot(e1, pv)
        inv = F(1) / np.where(det >= F(1.0e-25), det, F(1.0e-25))           # max(det, 1e-25) as the text's Max: a if a >= b else b
        v = dot(tv, pv) * inv
        u = dot(qv, d) * inv
        t = dot(e2, qv) * inv
    assert t.dtype == F and u.dtype == F and v.dtype == F
    return t, u, v


def scan_records(words, u=None, v=None):
    """The scan's records [n, 11] (int32 words in the layout above, words 9 and 10 whatever the scan keeps there) with u, v put in
    their place (None: 0, a scan that found no triangle)."""
    w = np.array(words, np.int32).reshape(-1, WORDS)
    w[:, U] = 0 if u is None else np.asarray(u, F).view(np.int32)
    w[:, V] = 0 if v is None else np.asarray(v, F).view(np.int32)
    return w


def records(o, d, tnear, tfar, scan):
    """-> (records [n, 11] int32, occluded [n] bool).  scan: scan_records() of the closest hits of shifted(o, d, tnear, tfar)[0] along d."""
    _, f, t0, live = shifted(o, d, tnear, tfar)
    scan = np.asarray(scan, np.int32).reshape(-1, WORDS)
    assert scan.shape[0] == f.shape[0]
    ts = scan[:, T].view(F)
    hit = live & (scan[:, IS_HIT] == 1) & (ts < f)
    out = np.zeros((len(f), WORDS), np.int32)                                # normal, u, v of a miss: +0
    out[:, T] = f.view(np.int32)                                             # a miss holds the bound
    out[:, PRIM_TYPE:MAT + 1] = -1
    with np.errstate(over="ignore", invalid="ignore"):
        t = (t0 + ts).astype(F)
    out[hit] = scan[hit]
    out[hit, T] = t[hit].view(np.int32)
    out[hit, IS_HIT] = 1
    return out, hit
