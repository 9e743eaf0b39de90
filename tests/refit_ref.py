"""Reference refit in plain numpy: what art_refit_device must leave in the exported tree, computed from the tree exported BEFORE the
refit, the mesh's index triples and the new positions.  Written from the header comments (csrc/art_scene.h node / record layout,
csrc/art_bvh.h child-box rule, csrc/art_qnode.h 8-bit snapping, csrc/art_refit.hip bad-vertex rule); it calls into none of the
project's libraries.  Every operation is a binary32 operation of numpy (numpy never contracts a multiply-add), vectorised per level.

  triangle record   words 0..8 = the three corners of primitive (word 9) at the new positions; words 9..11 unchanged
  leaf slot         tight box = min / max over the corners of its records
  inner slot        tight box = union of the tight boxes of the child node's good slots
  child box         tight box padded per axis by inflate_abs + inflate_rel * max(|l|, |h|), then one ulp outward
  width 4           the node's good child boxes snapped outward to the node's 8-bit grid, the dequantised planes are the tree
  bad slot          a leaf slot with a record coordinate that is not finite or beyond MAX_COORD in magnitude, or an inner slot whose child
                    node has no good slot: all six planes +inf, left out of the node's union and of the node's grid; reference word
                    and count word unchanged
  empty slot        (reference word < 0) untouched"""
import numpy as np

F = np.float32
INFLATE_REL = F(8.0e-6)      # BvhBuildParams::inflate_rel (art_bvh.h)
INFLATE_ABS = F(1.0e-6)      # BvhBuildParams::inflate_abs
MAX_COORD = F(1.0e18)        # kRefitMaxCoord (art_refit.h)
MAX_LEAF_TRIS = 8            # kMaxLeafTris (art_scene.h)
TINY = F(1.401298464e-45)    # the smallest positive binary32 value


def next_dn(v):
    """The binary32 neighbour below v (finite v); below +-0 lies the smallest negative subnormal."""
    v = np.asarray(v, F)
    b = v.view(np.int32)
    return np.where(v == 0, -TINY, (b + np.where(v > 0, -1, 1).astype(np.int32)).view(F))


def next_up(v):
    v = np.asarray(v, F)
    b = v.view(np.int32)
    return np.where(v == 0, TINY, (b + np.where(v > 0, 1, -1).astype(np.int32)).view(F))


def pad_box(l, h, inflate_rel=INFLATE_REL, inflate_abs=INFLATE_ABS):
    """art_bvh.h: pad = inflate_abs + inflate_rel * max(|l|, |h|) (a product, then a sum: two roundings), subtracted / added, one ulp outward."""
    l = np.asarray(l, F); h = np.asarray(h, F)
    pad = F(inflate_abs) + F(inflate_rel) * np.maximum(np.abs(l), np.abs(h))
    assert pad.dtype == F
    return next_dn(l - pad), next_up(h + pad)


def pow2_at_least(r):
    """Smallest power of two >= r (r > 0, normal)."""
    b = np.asarray(r, F).view(np.uint32)
    e = (b >> np.uint32(23)) + ((b & np.uint32(0x007fffff)) != 0).astype(np.uint32)
    return (e << np.uint32(23)).view(F)


def _grid(k, s, o):
    """fma(float(k), s, o) in binary32.  k is an integer <= 256 and s a power of two >= 2^-108, so k * s is exact in binary32 and the
    fma is ONE rounded addition of two binary32 values; the sum formed in binary64 and rounded to binary32 is that same value (double
    rounding is harmless for a single addition when the wide format has at least 2 * 24 + 2 bits, and binary64 has 53)."""
    ks = k.astype(F) * s
    return (ks.astype(np.float64) + o.astype(np.float64)).astype(F)


def quantise(lo, hi, good, codes=False):
    """art_qnode.h for n nodes at once.  lo, hi: [n, W, 3] padded boxes, good: [n, W] slots that take part.  Returns the dequantised
    planes (only entries under `good` mean anything) and the per-node origin and scale; with codes also the 8-bit plane numbers
    (ql, qh: int64 [n, W, 3])."""
    n, W, _ = lo.shape
    g3 = good[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        o = np.where(g3, lo, F(np.inf)).min(axis=1)                              # per-axis minimum of the good slots' lo ...
        o = np.where(good.any(axis=1)[:, None], o, F(0.0)).astype(F)             # ... (0 when the node has none)
        ext = np.where(g3, hi - o[:, None, :], F(0.0)).max(axis=(1, 2)).astype(F)
        ext = np.maximum(ext, F(0.0))
        s = pow2_at_least(np.maximum(ext, F(1.0e-30)) / F(255.0))
        ql = np.zeros((n, W, 3), np.int64); qh = np.zeros((n, W, 3), np.int64)
        todo = np.nonzero(good.any(axis=1))[0]
        rounds = 0
        while todo.size:
            ss = s[todo][:, None, None]; oo = np.broadcast_to(o[todo][:, None, :], (todo.size, W, 3)); gg = np.broadcast_to(g3[todo], (todo.size, W, 3))
            llo = np.where(gg, lo[todo], oo); hhi = np.where(gg, hi[todo], oo)
            k = np.clip(np.trunc((llo - oo) / ss), 0, 255).astype(np.int64)
            while True:                                                          # floor, corrected: the plane must not lie above lo
                dec = (k > 0) & (_grid(k, ss, oo) > llo)
                if not dec.any():
                    break
                k -= dec
            m = np.maximum(np.trunc((hhi - oo) / ss), 0).astype(np.int64)
            while True:                                                          # ceil, corrected: the plane must not lie below hi
                inc = (m <= 255) & (_grid(np.minimum(m, 255), ss, oo) < hhi)
                if not inc.any():
                    break
                m += inc
            fits = (m <= 255).all(axis=(1, 2))
            ql[todo[fits]] = k[fits]; qh[todo[fits]] = m[fits]
            s[todo[~fits]] = s[todo[~fits]] * F(2.0)                             # doubled until every plane fits
            todo = todo[~fits]
            rounds += 1
            assert rounds < 300, "the scale loop does not end"
        s3 = s[:, None, None]; o3 = np.broadcast_to(o[:, None, :], (n, W, 3))
        if codes:
            return _grid(ql, s3, o3), _grid(qh, s3, o3), o, s, ql, qh
        return _grid(ql, s3, o3), _grid(qh, s3, o3), o, s


def levels(nodes, W):
    """Node indices by depth, root first."""
    nodes = np.asarray(nodes, F).reshape(-1, 8 * W)
    ref = nodes[:, 3:4 * W:4].view(np.int32); cnt = nodes[:, 4 * W + 3:8 * W:4].view(np.int32)
    out = [np.array([0], np.int64)]
    while True:
        f = out[-1]
        kids = ref[f][(ref[f] >= 0) & (cnt[f] == 0)]
        if kids.size == 0:
            return out
        out.append(kids.astype(np.int64))
        assert len(out) <= nodes.shape[0]


def refit(nodes, tris, width, idx, pos, inflate_rel=INFLATE_REL, inflate_abs=INFLATE_ABS, quantised=None):
    """Expected (nodes, tris) after a refit to `pos`, both flat binary32 arrays like Backend.export_bvh() returns them.
    quantised: whether the tree's boxes are snapped to the 8-bit grid (default: exactly at width 4)."""
    W = int(width)
    quantised = (W == 4) if quantised is None else bool(quantised)
    nodes = np.array(nodes, F).reshape(-1, 8 * W); tris = np.array(tris, F).reshape(-1, 12)
    idx = np.asarray(idx, np.int32).reshape(-1, 3); pos = np.asarray(pos, F).reshape(-1, 3)
    N, n = nodes.shape[0], tris.shape[0]
    prim = tris[:, 9].view(np.int32)
    known = (prim >= 0) & (prim < idx.shape[0])
    tris[known, :9] = pos[idx[prim[known]]].reshape(-1, 9)
    c = tris[:, :9].reshape(n, 3, 3)
    with np.errstate(invalid="ignore"):
        rec_ok = (np.abs(tris[:, :9]) <= MAX_COORD).all(axis=1)                  # (false for NaN and +-inf)
        rlo = np.fmin.reduce(c, axis=1); rhi = np.fmax.reduce(c, axis=1)         # (values of bad records are never used)

    ref = nodes[:, 3:4 * W:4].view(np.int32).copy(); cnt = nodes[:, 4 * W + 3:8 * W:4].view(np.int32).copy()
    used = ref >= 0
    leaf = used & (cnt > 0); inner = used & (cnt == 0)
    tight_lo = np.full((N, 3), np.inf, F); tight_hi = np.full((N, 3), -np.inf, F)
    node_good = np.zeros(N, bool)
    lo_view = nodes[:, :4 * W].reshape(N, W, 4); hi_view = nodes[:, 4 * W:].reshape(N, W, 4)
    for lvl in reversed(levels(nodes, W)):
        m = lvl.size
        l = np.full((m, W, 3), np.inf, F); h = np.full((m, W, 3), -np.inf, F)
        r, k, lf, inn = ref[lvl], cnt[lvl], leaf[lvl], inner[lvl]
        bad = np.zeros((m, W), bool)
        for q in range(MAX_LEAF_TRIS):
            sel = lf & (k > q)
            if sel.any():
                t = r[sel] + q
                l[sel] = np.minimum(l[sel], rlo[t]); h[sel] = np.maximum(h[sel], rhi[t])
                bad[sel] |= ~rec_ok[t]
        l[inn] = tight_lo[r[inn]]; h[inn] = tight_hi[r[inn]]
        bad[inn] = ~node_good[r[inn]]
        good = used[lvl] & ~bad
        g3 = good[:, :, None]
        with np.errstate(invalid="ignore"):
            tight_lo[lvl] = np.where(g3, l, F(np.inf)).min(axis=1); tight_hi[lvl] = np.where(g3, h, F(-np.inf)).max(axis=1)
            node_good[lvl] = good.any(axis=1)
            plo, phi = pad_box(np.where(g3, l, F(0.0)), np.where(g3, h, F(0.0)), inflate_rel, inflate_abs)
        if quantised:
            plo, phi, _, _ = quantise(plo, phi, good)
        b3 = bad[:, :, None]
        new_lo = np.where(b3, F(np.inf), plo); new_hi = np.where(b3, F(np.inf), phi)
        keep = ~used[lvl][:, :, None]                                            # empty slots stay as the builder wrote them
        lo_view[lvl, :, :3] = np.where(keep, lo_view[lvl, :, :3], new_lo)
        hi_view[lvl, :, :3] = np.where(keep, hi_view[lvl, :, :3], new_hi)
    return nodes.reshape(-1), tris.reshape(-1)


def surviving_records(nodes, tris, width):
    """Records a ray can still reach: those of leaf slots whose six planes are finite, under inner slots whose planes are finite, from the
    root down.  Boolean mask over the triangle records."""
    W = int(width)
    nodes = np.asarray(nodes, F).reshape(-1, 8 * W); n = np.asarray(tris, F).reshape(-1, 12).shape[0]
    ref = nodes[:, 3:4 * W:4].view(np.int32); cnt = nodes[:, 4 * W + 3:8 * W:4].view(np.int32)
    N = nodes.shape[0]
    fin = np.isfinite(nodes[:, :4 * W].reshape(N, W, 4)[:, :, :3]).all(axis=2) & np.isfinite(nodes[:, 4 * W:].reshape(N, W, 4)[:, :, :3]).all(axis=2)
    alive = np.zeros(n, bool)
    frontier = np.array([0], np.int64)
    while frontier.size:
        ok = (ref[frontier] >= 0) & fin[frontier]
        lf = ok & (cnt[frontier] > 0)
        for q in range(MAX_LEAF_TRIS):
            sel = lf & (cnt[frontier] > q)
            alive[ref[frontier][sel] + q] = True
        frontier = ref[frontier][ok & (cnt[frontier] == 0)].astype(np.int64)
    return alive


def diff_report(got, want, what):
    """Assertion text in the style of the refit tests: the number and the first index of differing words."""
    got = np.asarray(got).reshape(-1).view(np.uint32); want = np.asarray(want).reshape(-1).view(np.uint32)
    assert got.size == want.size, "%s: %d words, expected %d" % (what, got.size, want.size)
    d = np.nonzero(got != want)[0]
    assert d.size == 0, "%d of %d %s words differ, first at word %d: got %08x (%r), want %08x (%r)" % (
        d.size, got.size, what, int(d[0]), int(got[d[0]]), float(got[d[:1]].view(F)[0]), int(want[d[0]]), float(want[d[:1]].view(F)[0]))
