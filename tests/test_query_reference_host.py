"""The rule the device-resident ray queries are held to (tests/query_ref.py) on hand-planted cases: the hits of the "scan" are arrays
written here, so the interval rule itself -- the shift, the bound, the strict comparison, the two record layouts -- is pinned without a
GPU and without the oracle library.  Every expectation below is written out by hand from include/art_hip.h, not computed by query_ref."""
import numpy as np

import ada_transcription as ada
import query_ref as Q

F = np.float32
FLT_MAX = F(3.4028234663852886e38)
MISS_IDS = [-1, -1, -1, -1]


def bits(x):
    return int(np.asarray(x, F).view(np.int32))


def planted(t, is_hit=1, prim_type=1, prim_index=5, mat_id=0, mat=7, normal=(0.0, 1.0, 0.0), u=0.0, v=0.0, texture=(0.25, 0.75)):
    """one record as the scan leaves it: its words 9, 10 hold texture coordinates, which must not reach the ArtHit"""
    w = [bits(t), is_hit, prim_type, prim_index, mat_id, mat] + [bits(c) for c in normal] + [bits(texture[0]), bits(texture[1])]
    return Q.scan_records(np.array([w], np.int32), u=[u], v=[v])


def one(o, d, tnear, tfar, scan):
    arr = lambda x: None if x is None else np.array([x], F)
    rec, occ = Q.records(np.array([o], F), np.array([d], F), arr(tnear), arr(tfar), scan)
    assert rec.shape == (1, 11) and rec.dtype == np.int32 and occ.shape == (1,) and occ.dtype == np.bool_
    return rec[0].tolist(), bool(occ[0])


O, D = (1.0, 2.0, 3.0), (0.0, 0.6, 0.8)


def hit_words(t, normal=(0.0, 1.0, 0.0), u=0.0, v=0.0):
    return [bits(t), 1, 1, 5, 0, 7] + [bits(c) for c in normal] + [bits(u), bits(v)]


def miss_words(bound):
    return [bits(bound), 0] + MISS_IDS + [0, 0, 0, 0, 0]


def test_no_interval_is_the_scan_itself_and_a_miss_holds_float_last():
    assert one(O, D, None, None, planted(2.5)) == (hit_words(2.5), True)
    # what the scan leaves in a record that is no hit (the oracle: the first candidate's fields) never shows
    assert one(O, D, None, None, planted(1.0, is_hit=0, prim_type=-1, prim_index=0, mat=3)) == (miss_words(FLT_MAX), False)


def test_negative_and_zero_tnear_shift_nothing():
    for tn in (-3.0, -0.0, 0.0, float("nan")):
        os_, f, t0, live = Q.shifted([O], [D], [tn], [10.0])
        assert os_.tolist() == [list(O)] and bits(f[0]) == bits(10.0) and bits(t0[0]) == 0 and live[0]
        assert one(O, D, tn, 10.0, planted(2.5)) == (hit_words(2.5), True)
    # without tnear the origin is not touched at all: -0 stays -0 (o + 0 * d would make it +0)
    os_, _, _, _ = Q.shifted([(-0.0, 0.0, 0.0)], [(1.0, 0.0, 0.0)])
    assert np.signbit(os_[0, 0])


def test_positive_tnear_shifts_by_a_rounded_multiply_and_a_rounded_add():
    o, d, tn = (F(0.1), F(1.0), F(-2.0)), (F(0.3), F(-0.7), F(0.1)), F(1.7)
    os_, f, t0, live = Q.shifted([o], [d], [tn], [4.0])
    for k in range(3):
        prod = F(np.float64(tn) * np.float64(d[k]))                   # binary64 holds the 48-bit product exactly: one rounding
        want = F(np.float64(o[k]) + np.float64(prod))                 # ... and the sum of two binary32 exactly: one rounding
        assert bits(os_[0, k]) == bits(want)
    fused = [F(np.float64(tn) * np.float64(d[k]) + np.float64(o[k])) for k in range(3)]
    assert any(bits(fused[k]) != bits(os_[0, k]) for k in range(3))  # (this case tells the two roundings from a fused multiply-add)
    assert bits(f[0]) == bits(F(4.0) - F(1.7)) and bits(t0[0]) == bits(1.7) and live[0]
    # the hit's t is t0 + t' rounded once; the bound it is held to is tfar - t0
    rec, occ = one(o, d, tn, 4.0, planted(0.3))
    assert rec == hit_words(F(1.7) + F(0.3)) and occ
    rec, occ = one(o, d, tn, 4.0, planted(2.4))                       # 2.4 > 4.0 - 1.7
    assert rec == miss_words(F(4.0) - F(1.7)) and not occ


def test_tfar_equal_to_tnear_is_empty():
    rec, occ = one(O, D, 1.5, 1.5, planted(0.25))
    assert rec == miss_words(0.0) and not occ                          # the bound of the empty interval: +0


def test_tfar_below_tnear_is_empty_and_reports_the_negative_bound():
    rec, occ = one(O, D, 2.0, 0.5, planted(0.25))
    assert rec == miss_words(-1.5) and not occ
    rec, occ = one(O, D, None, -1.0, planted(0.25))                    # no tnear, a negative tfar
    assert rec == miss_words(-1.0) and not occ
    rec, occ = one(O, D, -4.0, 0.0, planted(0.25))                     # tnear < 0 counts as 0: [0, 0] is empty
    assert rec == miss_words(0.0) and not occ


def test_a_nan_bound_is_empty():
    rec, occ = one(O, D, None, float("nan"), planted(0.25))
    assert not occ and rec[1:] == miss_words(0.0)[1:] and np.isnan(np.array([rec[0]], np.int32).view(F)[0])


def test_tfar_float_last():
    assert one(O, D, None, FLT_MAX, planted(2.5)) == (hit_words(2.5), True)
    assert one(O, D, None, FLT_MAX, planted(1.0, is_hit=0)) == (miss_words(FLT_MAX), False)
    # Float'Last - 2.5 rounds back to Float'Last: the miss still holds it, a hit adds t0 back
    assert one(O, D, 2.5, FLT_MAX, planted(1.0, is_hit=0)) == (miss_words(FLT_MAX), False)
    assert one(O, D, 2.5, None, planted(1.0, is_hit=0)) == (miss_words(FLT_MAX), False)
    assert one(O, D, 2.5, FLT_MAX, planted(4.0)) == (hit_words(6.5), True)


def test_a_hit_at_the_bound_is_a_miss_and_one_ulp_below_it_a_hit():
    f = F(3.25)
    below = np.nextafter(f, F(0))
    rec, occ = one(O, D, None, f, planted(f))
    assert rec == miss_words(f) and not occ
    rec, occ = one(O, D, None, f, planted(below))
    assert rec == hit_words(below) and occ
    # with a shift the comparison is t' against tfar - t0, not t0 + t' against tfar: here fl(t0 + t') == tfar although t' < f
    t0, tfar = F(1.0), F(1.0) + F(2.0) ** -23                          # f = 2^-23
    tp = F(2.0) ** -23 - F(2.0) ** -47                                 # one ulp below f; 1 + t' rounds up to tfar
    assert tp < tfar - t0 and bits(t0 + tp) == bits(tfar)
    rec, occ = one(O, D, t0, tfar, planted(tp))
    assert rec == hit_words(tfar) and occ
    rec, occ = one(O, D, t0, tfar, planted(F(2.0) ** -23))
    assert rec == miss_words(F(2.0) ** -23) and not occ


def test_a_triangle_hit_keeps_ids_normal_and_barycentrics_and_drops_the_texture_words():
    n = (F(0.1), F(-0.2), F(0.97))
    scan = planted(0.75, prim_type=2, prim_index=1234, mat_id=9, mat=9, normal=n, u=0.125, v=0.5, texture=(0.3, 0.6))
    rec, occ = one(O, D, 0.5, 2.0, scan)
    assert rec == [bits(1.25), 1, 2, 1234, 9, 9, bits(n[0]), bits(n[1]), bits(n[2]), bits(0.125), bits(0.5)] and occ
    rec, occ = one(O, D, 0.5, 1.25, scan)                              # f = 0.75 == t': beyond the bound; nothing of the triangle is left
    assert rec == miss_words(0.75) and not occ


def test_rays_of_one_call_are_independent():
    """the planted cases above in one call: each record is what the case gave alone"""
    cases = [(None, None, planted(2.5)), (1.5, 1.5, planted(0.25)), (2.0, 0.5, planted(0.25)), (0.5, 3.0, planted(2.5)), (-1.0, 3.0, planted(2.5)),
             (0.0, FLT_MAX, planted(1.0, is_hit=0)), (0.5, 3.0, planted(2.0))]
    tn = np.array([0.0 if c[0] is None else c[0] for c in cases], F)
    tf = np.array([FLT_MAX if c[1] is None else c[1] for c in cases], F)
    scan = np.concatenate([c[2] for c in cases])
    n = len(cases)
    rec, occ = Q.records(np.tile(F(O), (n, 1)), np.tile(F(D), (n, 1)), tn, tf, scan)
    for i, (a, b, s) in enumerate(cases):
        want, wocc = one(O, D, tn[i], tf[i], s)
        assert rec[i].tolist() == want and bool(occ[i]) == wocc
    assert occ.tolist() == [True, False, False, False, True, False, True]


def test_barycentrics_equal_the_scalar_transcription_of_the_ada_text():
    """the vectorised Moeller-Trumbore of query_ref against tests/ada_transcription.py intersect_triangle, ray by ray, bit for bit"""
    rng = np.random.default_rng(5)
    n = 400
    A, B, C = (rng.normal(0, 1, (n, 3)).astype(F) for _ in range(3))
    w = rng.dirichlet([1, 1, 1], n)
    p = (w[:, :1] * A + w[:, 1:2] * B + w[:, 2:] * C)
    o = (p + rng.normal(0, 2, (n, 3))).astype(F)
    d = p - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    t, u, v = Q.barycentrics(o, d, A, B, C)
    seen = 0
    for i in range(n):
        h = ada.intersect_triangle(tuple(o[i]), tuple(d[i]), tuple(A[i]), tuple(B[i]), tuple(C[i]), F(0), F(1.0e6))
        if h["is_hit"]:
            seen += 1
            assert (bits(t[i]), bits(u[i]), bits(v[i])) == (bits(h["tmin"]), bits(h["u"]), bits(h["v"]))
    assert seen > n // 4                                               # (front faces: the text rejects the others through its clamped determinant)
