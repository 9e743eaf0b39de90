"""Reference updates of an instanced scene in plain numpy: what art_move_instances_device and art_refit_mesh_device must leave in every
array Backend.export_two_level() returns, computed from the export taken BEFORE the update and the update's inputs.  Written from the
header comments (csrc/art_move.hip: the order and the rules of the update; csrc/art_instanced_build.cpp: invert_3x4, world_box, the pad
bound; csrc/art_refit_node.h: a node refit; csrc/art_qnode.h: the quantised node; csrc/art_scene.h: DevInstance); it calls into none of
the project's libraries, and the node arithmetic is tests/refit_ref.py's (pad_box, quantise, levels, and refit itself as a cross-check).

  matrices     DevInstance::m = the input; minv = invert_3x4 in binary64, rounded once (zeros where there is no inverse).  An instance is
               BAD when an element is not finite, the determinant fails invert_3x4's test, or a row reaches beyond MAX_REACH:
               reach_r = |m_r3| + sum_j |m_rj| * max(|box.lo_j|, |box.hi_j|) over its mesh's object-space box
  extent       E = max(the scene's extent without the instances, the good instances' reaches)
  pads         needed[mesh] = max over its good instances and rows of 8 * 2^-24 * ((|q0| + |q1| + |q2|) * 3 E + |q3|), q = the stored minv row;
               pad = max(mesh_pad_min, binary32(min(needed, 1e30))); a mesh's pad only grows, and a mesh whose pad grew has every node
               refitted with it (refit_ref's rules; the tight boxes are those of its records as they are)
  entry point  the box of the corners of the records below root_entry under m: binary64 products and sums in world_box's order, the
               four-term pad, one rounding; written to its proxy record's nine words.  Empty (the proxy keeps its words) for a bad
               instance or a record with a bad coordinate
  instance     level by level, deepest first: a leaf child's box is the union of its proxies' entry boxes, an inner child's the tight
  tree         union below; nothing good below = a bad child (planes +inf); good children padded by the builder's default rule
  quantised    c0 = lo.x | lo.y << 8 | lo.z << 16 | hi.x << 24, c1 = hi.y | hi.z << 8 (bad or empty child: 0x00ffffff, 0), the header words
  nodes        origin and scale; every entry word as before
  mesh refit   the mesh's records take the new corners (refit_ref), its tree is refitted under the pad in force, its box becomes the tight box
               of its root (kept when that is empty), and everything above runs at the matrices in force"""
import numpy as np

import refit_ref
from refit_ref import F, levels, next_dn, next_up, pad_box, quantise      # noqa: F401  (next_dn / next_up: the pad rule's, through pad_box)

MAX_REACH = 1.0e18           # kMoveMaxReach (art_move.h)
NODE_BASE, TRI_BASE, SHADE_BASE, ROOT_ENTRY, QROOT, INST = 24, 25, 26, 27, 28, 29      # DevInstance words (m: 0..11, minv: 12..23)
ARRAYS = ("inst", "tlas_nodes", "tlas_tris", "blas_nodes", "blas_tris", "qnodes", "mesh_pad", "mesh_box", "mesh_base", "node_mesh")
INF = F(np.inf)


def invert_3x4(m):
    """art_instanced_build.cpp invert_3x4, expression for expression: (has an inverse, the 12 binary32 words)"""
    m = [float(v) for v in np.asarray(m, F)]
    a, b, c, d, e, f, g0, h, i = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
    out = np.zeros(12, F)
    det = a * (e * i - f * h) - b * (d * i - f * g0) + c * (d * h - e * g0)
    if not (abs(det) > 1.0e-300) or not np.isfinite(det):
        return False, out
    with np.errstate(over="ignore", invalid="ignore"):
        det = np.float64(det)
        r = [(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
             (f * g0 - d * i) / det, (a * i - c * g0) / det, (c * d - a * f) / det,
             (d * h - e * g0) / det, (b * g0 - a * h) / det, (a * e - b * d) / det]
        for row in range(3):
            for k in range(3):
                out[4 * row + k] = F(r[3 * row + k])
            out[4 * row + 3] = F(-(r[3 * row] * m[3] + r[3 * row + 1] * m[7] + r[3 * row + 2] * m[11]))
    return True, out


def reaches(m, box):
    """the three row reaches of matrix m over the object-space box (6 words), binary64"""
    m = [float(v) for v in np.asarray(m, F)]
    b = [float(v) for v in np.asarray(box, F)]
    out = []
    for r in range(3):
        reach = abs(m[4 * r + 3])
        for j in range(3):
            reach += abs(m[4 * r + j]) * max(abs(b[j]), abs(b[j + 3]))
        out.append(reach)
    return out


def refit_nodes(nodes, qn, rlo, rhi, rok, pad_rel, pad_abs, leaf_rule):
    """art_refit_node.h over a whole 4-wide tree (node 0 its root, references relative to it).  rlo, rhi [n, 3], rok [n]: box and state
    of record k.  leaf_rule "all": a leaf child is bad when one of its records is (a mesh's tree); "any": a bad record adds nothing
    and the child is bad when nothing is left (the instance tree).  Returns (packets, quantised nodes, tight lo, tight hi per node)."""
    W = 4
    nodes = np.array(nodes, F).reshape(-1, 32); qn = np.array(qn, np.uint32).reshape(-1, 16)
    N = nodes.shape[0]
    ref = nodes[:, 3:16:4].view(np.int32).copy(); cnt = nodes[:, 19:32:4].view(np.int32).copy()
    used = ref >= 0
    leaf = used & (cnt > 0); inner = used & (cnt == 0)
    tight_lo = np.full((N, 3), np.inf, F); tight_hi = np.full((N, 3), -np.inf, F)
    lo_view = nodes[:, :16].reshape(N, W, 4); hi_view = nodes[:, 16:].reshape(N, W, 4)
    q = qn.reshape(N, W, 4)
    for lvl in reversed(levels(nodes.reshape(-1), W)):
        m = lvl.size
        l = np.full((m, W, 3), np.inf, F); h = np.full((m, W, 3), -np.inf, F)
        r, k, lf, inn = ref[lvl], cnt[lvl], leaf[lvl], inner[lvl]
        rec_bad = np.zeros((m, W), bool)
        for t in range(refit_ref.MAX_LEAF_TRIS):
            sel = lf & (k > t)
            if sel.any():
                rr = r[sel] + t
                take = rok[rr][:, None] | (leaf_rule == "all")
                l[sel] = np.where(take, np.minimum(l[sel], rlo[rr]), l[sel]); h[sel] = np.where(take, np.maximum(h[sel], rhi[rr]), h[sel])
                rec_bad[sel] |= ~rok[rr]
        l[inn] = tight_lo[r[inn]]; h[inn] = tight_hi[r[inn]]
        empty = ~(l[:, :, 0] <= h[:, :, 0])
        bad = used[lvl] & ((lf & rec_bad) if leaf_rule == "all" else (lf & empty))
        bad |= inn & empty
        good = used[lvl] & ~bad
        g3 = good[:, :, None]
        with np.errstate(invalid="ignore"):
            tight_lo[lvl] = np.where(g3, l, INF).min(axis=1); tight_hi[lvl] = np.where(g3, h, -INF).max(axis=1)
            plo, phi = pad_box(np.where(g3, l, F(0.0)), np.where(g3, h, F(0.0)), pad_rel, pad_abs)
        plo, phi, o, s, ql, qh = quantise(plo, phi, good, codes=True)
        b3 = bad[:, :, None]
        keep = ~used[lvl][:, :, None]                                            # empty slots stay as the builder wrote them
        lo_view[lvl, :, :3] = np.where(keep, lo_view[lvl, :, :3], np.where(b3, INF, plo))
        hi_view[lvl, :, :3] = np.where(keep, hi_view[lvl, :, :3], np.where(b3, INF, phi))
        c0 = (ql[:, :, 0] | (ql[:, :, 1] << 8) | (ql[:, :, 2] << 16) | (qh[:, :, 0] << 24)).astype(np.uint32)
        c1 = (qh[:, :, 1] | (qh[:, :, 2] << 8)).astype(np.uint32)
        q[lvl, :, 0] = np.where(good, c0, np.uint32(0x00ffffff)); q[lvl, :, 1] = np.where(good, c1, np.uint32(0))
        hdr = np.concatenate([o, s[:, None]], axis=1).astype(F)                  # record j carries header word j: origin x, y, z, scale
        q[lvl, :, 3] = hdr.view(np.uint32)
    return nodes, qn, tight_lo, tight_hi


def _record_boxes(tris):
    t = np.asarray(tris, F).reshape(-1, 12)
    c = t[:, :9].reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(t[:, :9]) <= refit_ref.MAX_COORD).all(axis=1)
        return np.fmin.reduce(c, axis=1), np.fmax.reduce(c, axis=1), ok


def mesh_slices(S, mi):
    """(first node, node count, first record or -1, record count, first quantised node) of mesh mi"""
    at = np.nonzero(S["node_mesh"] == mi)[0]
    nb, tb, qb = (int(v) for v in S["mesh_base"][mi])
    assert at.size and at[0] == nb and at[-1] - at[0] + 1 == at.size, "a mesh's nodes are one after the other"
    nd = S["blas_nodes"][nb:nb + at.size]
    ref = nd[:, 3:16:4].view(np.int32); cnt = nd[:, 19:32:4].view(np.int32)
    lf = (ref >= 0) & (cnt > 0)
    return nb, int(at.size), tb, int((ref[lf] + cnt[lf]).max()), qb


def _refit_mesh_tree(S, mi, pad_abs):
    """mesh mi's nodes and quantised nodes under pad_abs, from its records as they are; returns the tight box of its root"""
    nb, nn, tb, nrec, qb = mesh_slices(S, mi)
    rlo, rhi, rok = _record_boxes(S["blas_tris"][tb:tb + nrec])
    before = S["blas_nodes"][nb:nb + nn].copy()
    nodes, qn, tlo, thi = refit_nodes(before, S["qnodes"][qb:qb + nn], rlo, rhi, rok, S["mesh_pad_rel"], pad_abs, "all")
    want, _ = refit_ref.refit(before.reshape(-1), S["blas_tris"][tb:tb + nrec].reshape(-1), 4, np.zeros((0, 3), np.int32), np.zeros((0, 3), F),
                              S["mesh_pad_rel"], pad_abs)                        # the flat refit's reference gives the same packets
    assert np.array_equal(nodes.reshape(-1).view(np.uint32), want.view(np.uint32)), "two_level_ref and refit_ref disagree on a mesh's packets"
    S["blas_nodes"][nb:nb + nn] = nodes; S["qnodes"][qb:qb + nn] = qn
    return tlo[0], thi[0]


def records_below(S, node_base, tri_base, root_entry):
    """indices into blas_tris of the records below an entry word of a mesh's tree"""
    nodes = S["blas_nodes"]
    out, stack = [], [int(root_entry)]
    while stack:
        w = stack.pop()
        ref, cnt = w >> 4, w & 15
        if cnt:
            out.extend(range(tri_base + ref, tri_base + ref + cnt))
            continue
        nd = nodes[node_base + ref]
        for j in range(4):
            rj = int(nd[4 * j + 3:4 * j + 4].view(np.int32)[0])
            if rj >= 0:
                stack.append((rj << 4) | int(nd[16 + 4 * j + 3:16 + 4 * j + 4].view(np.int32)[0]))
    return np.array(sorted(out), np.int64)


def entry_box(m, tris):
    """world_box of art_instanced_build.cpp over the corners of the records `tris` [n, 12] under matrix m: (lo, hi) binary32, or None
    when a coordinate is bad"""
    p32 = np.asarray(tris, F).reshape(-1, 12)[:, :9].reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        if not (np.abs(p32) <= refit_ref.MAX_COORD).all():
            return None
    p = p32.astype(np.float64)
    M = np.asarray(m, F).astype(np.float64)
    lo, hi = np.zeros(3, F), np.zeros(3, F)
    for r in range(3):
        a = M[4 * r] * p[:, 0]; b = M[4 * r + 1] * p[:, 1]; c = M[4 * r + 2] * p[:, 2]
        w = a + b + c + M[4 * r + 3]
        mag = float((np.abs(a) + np.abs(b) + np.abs(c) + abs(M[4 * r + 3])).max())
        l, h = float(w.min()), float(w.max())
        pad = 1.0e-4 * (h - l) + 1.0e-5 * max(abs(l), abs(h)) + 1.0e-6 * mag + 1.0e-6
        lo[r] = F(l - pad); hi[r] = F(h + pad)
    return lo, hi


def copy_of(ex):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ex.items()}


def _pipeline(S, m, dirty=()):
    """k_move_begin .. k_move_tlas_level at the matrices m [n_inst, 12]; dirty: meshes whose records changed (their trees are refitted
    whether their pad grows or not).  Returns S and what the reference knows besides the arrays."""
    m = np.ascontiguousarray(m, F).reshape(-1, 12)
    inst = S["inst"]
    n_inst, n_entry, nm = S["n_inst"], inst.shape[0], S["mesh_pad"].shape[0]
    assert m.shape[0] == n_inst
    base = [int(v) for v in S["mesh_base"][:, 0]]
    inst_mesh = [base.index(int(inst[i, NODE_BASE])) for i in range(n_inst)]
    # matrices, the extent
    ok = np.zeros(n_inst, bool); minv = np.zeros((n_inst, 12), F)
    E = float(S["scene_extent"])
    for i in range(n_inst):
        fin = bool(np.isfinite(m[i]).all())
        inv = False
        if fin:
            inv, minv[i] = invert_3x4(m[i])
        with np.errstate(invalid="ignore", over="ignore"):
            rs = reaches(m[i], S["mesh_box"][inst_mesh[i]])
        ok[i] = inv and all(r <= MAX_REACH for r in rs)
        if ok[i]:
            E = max(E, max(rs))
    owner = inst[:, INST].view(np.int32)
    inst[:, 0:12] = m[owner].view(np.uint32); inst[:, 12:24] = minv[owner].view(np.uint32)
    # pads
    needed = [0.0] * nm
    for i in np.nonzero(ok)[0]:
        q = [float(v) for v in minv[i]]
        for r in range(3):
            bound = 8.0 * 5.9604644775390625e-8 * ((abs(q[4 * r]) + abs(q[4 * r + 1]) + abs(q[4 * r + 2])) * 3.0 * E + abs(q[4 * r + 3]))
            if np.isfinite(bound):
                needed[inst_mesh[i]] = max(needed[inst_mesh[i]], bound)
    repadded = []
    for mi in range(nm):
        nf = max(F(S["mesh_pad_min"]), F(min(needed[mi], 1.0e30)))
        if nf > S["mesh_pad"][mi]:
            S["mesh_pad"][mi] = nf; repadded.append(mi)
    for mi in sorted(set(repadded) | set(dirty)):
        if S["mesh_base"][mi, 1] >= 0:                                           # (a mesh nobody shows is never touched)
            _refit_mesh_tree(S, mi, S["mesh_pad"][mi])
    # entry points
    elo = np.full((n_entry, 3), np.inf, F); ehi = np.full((n_entry, 3), -np.inf, F)
    proxy_of = np.full(n_entry, -1, np.int64)
    ids = S["tlas_tris"][:, 9].view(np.int32)
    proxy_of[ids] = np.arange(ids.size)
    assert (proxy_of >= 0).all() and ids.size == n_entry, "one proxy per entry point"
    below = {}
    for e in range(n_entry):
        if not ok[owner[e]]:
            continue
        key = (int(inst[e, NODE_BASE]), int(inst[e, TRI_BASE]), int(inst[e, ROOT_ENTRY].view(np.int32)))
        if key not in below:
            below[key] = records_below(S, *key)
        box = entry_box(m[owner[e]], S["blas_tris"][below[key]])
        if box is None:
            continue
        elo[e], ehi[e] = box
        S["tlas_tris"][proxy_of[e], :9] = [box[0][0], box[0][1], box[0][2], box[1][0], box[1][1], box[1][2], box[0][0], box[1][1], box[0][2]]
    # the instance tree
    n_tlas = S["tlas_nodes"].shape[0]
    eok = elo[:, 0] <= ehi[:, 0]
    nodes, qn, _, _ = refit_nodes(S["tlas_nodes"], S["qnodes"][:n_tlas], elo[ids], ehi[ids], eok[ids], S["tlas_pad_rel"], S["tlas_pad_abs"], "any")
    S["tlas_nodes"][:] = nodes; S["qnodes"][:n_tlas] = qn
    S["updated"] = 1
    return S, dict(ok=ok, E=E, repadded=repadded, entry_lo=elo, entry_hi=ehi, inst_mesh=inst_mesh)


def move(ex, m, details=False):
    """the export after art_move_instances_device(m)"""
    S, d = _pipeline(copy_of(ex), m)
    return (S, d) if details else S


def refit_mesh(ex, mesh, idx, pos, details=False):
    """the export after art_refit_mesh_device(mesh, pos): idx are the mesh's index triples"""
    S = copy_of(ex)
    idx = np.asarray(idx, np.int32).reshape(-1, 3); pos = np.asarray(pos, F).reshape(-1, 3)
    nb, nn, tb, nrec, qb = mesh_slices(S, mesh)
    assert tb >= 0, "no instance shows the mesh"
    rec = S["blas_tris"][tb:tb + nrec]
    prim = rec[:, 9].view(np.int32)
    assert ((prim >= 0) & (prim < idx.shape[0])).all()
    rec[:, :9] = pos[idx[prim]].reshape(-1, 9)
    tlo, thi = _refit_mesh_tree(S, mesh, S["mesh_pad"][mesh])                   # under the pad in force; the pipeline may widen it
    if tlo[0] <= thi[0]:
        S["mesh_box"][mesh] = np.concatenate([tlo, thi])
    S, d = _pipeline(S, S["inst"][:S["n_inst"], 0:12].view(F).copy(), dirty=(mesh,))
    return (S, d) if details else S


def tlas_levels(ex):
    return len(levels(ex["tlas_nodes"].reshape(-1), 4))


def assert_equal(got, want, what):
    """every exported array, word for word"""
    for name in ARRAYS:
        refit_ref.diff_report(got[name], want[name], "%s: %s" % (what, name))
