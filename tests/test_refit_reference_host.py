"""The reference refit (tests/refit_ref.py) is checked on the CPU before any GPU test relies on it:
  * its pieces against exact arithmetic (the padding rule, the one-ulp steps, the 8-bit grid);
  * refitted to the uploaded positions it reproduces the host builder's tree word for word, at width 4 and width 8, on the soup, the
    structured mesh, the degenerate meshes and the 1- and 2-triangle meshes;
  * the bad-vertex rule on a tree small enough to state the expected planes by hand;
  * every shape case of tests/test_gpu_refit_reference.py: the reference tree of the moved mesh is sound, and the oracle's walk of it
    returns the brute-force hits -- so a surprise on the GPU is about the kernels."""
from fractions import Fraction

import numpy as np
import pytest

import bvh_check
import conv
import hostsim
import orc
import refit_ref

F = np.float32


def mesh_scene(art, pos, idx, nrm=None):
    """A scene of one CLOSEST mesh and nothing else a ray could hit (every ray starts unbounded)."""
    from ada_ray_tracer_amd import scenes
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3); idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    if nrm is None:
        nrm = np.tile(np.array([0, 1, 0], F), (pos.shape[0], 1))
    mesh = dict(mode=art.MESH_CLOSEST, pos=pos, nrm=np.ascontiguousarray(nrm, F), idx=idx, matid=(1 + np.arange(idx.shape[0]) % 3).astype(np.int32))
    light = [dict(shape=art.LIGHT_SPHERE, mat=4, center=(0.0, 40.5, 1.0), radius=0.5, intensity=(10.0, 10.0, 10.0), surfaceArea=3.14159)]
    return art.SceneDesc([], light, scenes.cornell_materials(), [mesh], None, scenes.REFERENCE_CAMERA)


def _soup(n, seed=0x5EED):
    from ada_ray_tracer_amd import scenes
    m = scenes.random_triangles(n, seed + n)
    return m["pos"], m["idx"]


def _grid(n):
    """The first n triangles of a regular grid: shared vertices, fewer vertices than triangles."""
    from ada_ray_tracer_amd import scenes
    m = 1
    while 2 * m * m < n:
        m += 1
    g = scenes.grid_mesh(m)
    idx = g["idx"][:n]
    return g["pos"][:int(idx.max()) + 1].copy(), idx.copy()


def _shift(pos, seed):
    """A translation, a small rotation-free shear and a jitter: every box of the tree changes."""
    rng = np.random.default_rng(seed)
    p = pos.astype(np.float64)
    p = p + np.array([0.21, -0.13, 0.17]) + 0.05 * p[:, [1, 2, 0]] + 2e-3 * rng.standard_normal(p.shape)
    return p.astype(F)


def _scaled(pos, target):
    """pos scaled about the origin so that its largest coordinate magnitude is `target` (never above it)."""
    p = pos.astype(np.float64) * (target / np.abs(pos.astype(np.float64)).max())
    q = p.astype(F)
    over = np.abs(q) > F(target)
    q[over] = np.copysign(F(target), q[over])
    return q


SHAPES = ["tri1", "tri2"] + ["%s%d" % (k, n) for k in ("soup", "grid") for n in (255, 256, 257, 513)] + \
         ["unreferenced", "point", "plane_y", "scale_1e-30", "scale_1e9", "scale_9e17", "neg_zero"]
# shape cases whose rays need not hit (the assertion there is that the tree matches and the hit set equals the oracle's): a point has no
# area, at 1e-30 the triangle test's products underflow, and at 9e17 neighbouring binary32 values lie 6.9e10 apart while the triangle
# test accepts 0 < t < 1e6 only (and its products overflow)
MAY_MISS = ("point", "scale_1e-30", "scale_9e17")


def shape_case(name):
    """(uploaded positions, index triples, positions the mesh is refitted to)."""
    if name in ("tri1", "tri2"):
        pos, idx = _soup(int(name[3:]))
        return pos, idx, _shift(pos, 1)
    if name.startswith("soup") or name.startswith("grid"):
        pos, idx = (_soup if name.startswith("soup") else _grid)(int(name[4:]))
        return pos, idx, _shift(pos, 2)
    pos, idx = _soup(300)
    if name == "unreferenced":
        rng = np.random.default_rng(3)
        pos = np.concatenate([pos, (rng.random((1000, 3)) * 4.0).astype(F)])
        return pos, idx, _shift(pos, 3)
    if name == "point":
        return pos, idx, np.tile(np.array([0.3, 2.0, 2.5], F), (pos.shape[0], 1))
    if name == "plane_y":
        new = _shift(pos, 4); new[:, 1] = F(2.0)
        return pos, idx, new
    if name.startswith("scale_"):
        return pos, idx, _scaled(_shift(pos, 5), float(name[6:]))
    if name == "neg_zero":
        new = _shift(pos, 6)
        new[0::2, 0] = F(-0.0); new[1::4, 0] = F(0.0); new[0::5, 2] = F(-0.0); new[2::7, 1] = F(-0.0)
        return pos, idx, new
    raise KeyError(name)


def rays_at(pos, idx, n, seed):
    """n rays built from the mesh's own bounds: from points at most 1.5 diagonals away (and within 4e5, the triangle test accepts
    t < 1e6 only) towards points inside its triangles, one in eight axis-parallel and one in eight in a random direction."""
    rng = np.random.default_rng(seed)
    p = np.asarray(pos, np.float64).reshape(-1, 3)
    tri = p[np.asarray(idx).reshape(-1, 3)]
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    dist = min(4.0e5, max(1.5 * float(np.linalg.norm(hi - lo)), 1e-3 * float(np.abs(tri).max()), 1e-37))
    t = tri[rng.integers(0, tri.shape[0], n)]
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    target = (t * w[:, :, None]).sum(1)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = n // 8
    if float(np.abs(tri).max()) + dist < 3.0e8:
        d[:k] = np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], (k, 1))
    o = target - dist * rng.uniform(0.3, 1.0, (n, 1)) * d
    d[k:2 * k] = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(o.astype(F)), np.ascontiguousarray(d.astype(F))


# ---- the pieces -----------------------------------------------------------------------------------------------------------------------
EDGE = np.array([0.0, -0.0, 1.401298464e-45, -1.401298464e-45, 1e-38, 1.17549435e-38, -1.17549435e-38, 1e-30, -1e-30, 1.0, -1.0, 0.1, 2.5,
                 -4.75, 1e9, -1e9, 9e17, -9e17, 1e18, -1e18, 16777216.0, 3.0e38], F)


def test_one_ulp_steps_are_the_neighbours():
    with np.errstate(over="ignore"):
        up = np.nextafter(EDGE, F(np.inf)); dn = np.nextafter(EDGE, F(-np.inf))
    assert np.array_equal(refit_ref.next_up(EDGE).view(np.uint32), up.view(np.uint32))
    assert np.array_equal(refit_ref.next_dn(EDGE).view(np.uint32), dn.view(np.uint32))


def test_padding_rule_against_exact_arithmetic():
    """pad = round(abs + round(rel * max(|l|, |h|))), lo = the neighbour below round(l - pad), hi = the neighbour above round(h + pad):
    every rounding done on exact rationals."""
    rng = np.random.default_rng(1)
    l = np.concatenate([EDGE[:-1], (rng.standard_normal(200) * 10.0 ** rng.integers(-30, 18, 200)).astype(F)])
    h = np.maximum(l, np.roll(l, 7))
    lo, hi = refit_ref.pad_box(l, h)
    for a, b, x, y in zip(l, h, lo, hi):
        m = max(abs(Fraction(float(a))), abs(Fraction(float(b))))
        prod = F(float(refit_ref.INFLATE_REL) * float(m))                         # binary64 product of two binary32 values is exact
        pad = F(float(refit_ref.INFLATE_ABS) + float(prod))
        want_lo = np.nextafter(F(float(a) - float(pad)), F(-np.inf)); want_hi = np.nextafter(F(float(b) + float(pad)), F(np.inf))
        assert x.view(np.uint32) == want_lo.view(np.uint32) and y.view(np.uint32) == want_hi.view(np.uint32), (a, b, x, y, want_lo, want_hi)
        assert x < a and y > b and pad > 0


def test_grid_encloses_and_is_the_smallest_that_fits():
    rng = np.random.default_rng(2)
    n = 400
    mag = 10.0 ** rng.integers(-30, 18, (n, 1, 1))
    c = rng.standard_normal((n, 4, 3)) * mag
    e = np.abs(rng.standard_normal((n, 4, 3))) * mag * 10.0 ** rng.integers(-6, 1, (n, 1, 1))
    lo = (c - e).astype(F); hi = (c + e).astype(F)
    lo[:20] = hi[:20] = F(0.75)                                                    # zero extent
    good = rng.random((n, 4)) < 0.8
    good[:, 0] = True
    qlo, qhi, o, s = refit_ref.quantise(lo, hi, good)
    g3 = np.broadcast_to(good[:, :, None], lo.shape)
    assert (qlo[g3] <= lo[g3]).all() and (qhi[g3] >= hi[g3]).all(), "the dequantised box does not enclose"
    assert np.array_equal(o, np.where(g3, lo, np.inf).min(1).astype(F))
    frac, _ = np.frexp(s)
    assert (frac == 0.5).all(), "the scale is not a power of two"
    ext = np.where(g3, hi.astype(np.float64) - o[:, None, :], 0.0).max(axis=(1, 2))
    wide = ext > 1e-30
    assert (s[wide].astype(np.float64) * 255.0 >= ext[wide] * (1 - 1e-6)).all(), "the planes cannot fit this scale"
    assert (s[wide].astype(np.float64) * 255.0 <= ext[wide] * 4.0 * (1 + 1e-6)).all(), "the scale is more than two doublings above extent / 255"
    # every plane is one of the node's 256 grid points fma(k, s, o), formed here in exact arithmetic and rounded once
    grid = (np.arange(256)[None, :, None] * s[:, None, None].astype(np.float64) + o[:, None, :].astype(np.float64)).astype(F)      # [n, 256, 3]
    for q in (qlo, qhi):
        on_grid = (q[:, :, None, :] == grid[:, None, :, :]).any(axis=2)
        assert on_grid[g3].all(), "a plane is not a grid point"


# ---- against the host builder --------------------------------------------------------------------------------------------------------
def _degenerate(name):
    rng = np.random.default_rng(5)
    tri = np.array([[-1, 1, 2], [1, 1, 2], [0, 3, 2.5]], F)
    tris = {
        "identical": np.tile(tri, (20000, 1, 1)),
        "zero_area": np.concatenate([np.tile(tri, (50, 1, 1)), np.tile(tri[:1], (3000, 3, 1))]),
        "wide_range": (rng.normal(size=(6000, 1, 3)) * 10.0 ** rng.integers(-3, 3, (6000, 1, 1)) + rng.normal(size=(6000, 3, 3)) * 0.05 + [0, 2, 2]).astype(F),
    }[name]                                                                       # (the meshes of test_gpu_degenerate.py)
    return tris.reshape(-1, 3), np.arange(3 * tris.shape[0], dtype=np.int32).reshape(-1, 3)


def _built_scene(art, name):
    from ada_ray_tracer_amd import scenes
    if name == "soup":
        sd = scenes.synthetic_scene(2000, 3)
    elif name == "structured":
        sd = scenes.structured_scene(20000)
    elif name in ("tri1", "tri2"):
        sd = mesh_scene(art, *_soup(int(name[3:])))
    else:
        sd = mesh_scene(art, *_degenerate(name))
    pos, _, idx, _, _ = sd._mesh_arrays[-1]
    return sd, pos, idx


@pytest.fixture
def host_width(art):
    yield lambda w: hostsim.set_bvh_param(art, "width", w)
    hostsim.set_bvh_param(art, "width", 4)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("name", ["soup", "structured", "identical", "zero_area", "wide_range", "tri1", "tri2"])
def test_reference_reproduces_the_host_builder(art, host_width, name, width):
    sd, pos, idx = _built_scene(art, name)
    host_width(width)
    nodes, tris, info = hostsim.bvh(art, sd)
    assert info["width"] == width and info["n_tris"] == idx.shape[0]
    want_nodes, want_tris = refit_ref.refit(nodes, tris, width, idx, pos)
    refit_ref.diff_report(want_tris, tris, "triangle record")
    refit_ref.diff_report(want_nodes, nodes, "node")
    # a reference that returned its input would pass the lines above: from a tree whose boxes were wiped it must rebuild the same planes
    wiped = nodes.copy().reshape(-1, 8 * width)
    used = wiped[:, 3:4 * width:4].view(np.int32) >= 0
    for a in range(3):
        wiped[:, a:4 * width:4][used] = F(123.0); wiped[:, 4 * width + a::4][used] = F(-123.0)
    stale = tris.copy().reshape(-1, 12); stale[:, :9] = F(7.0)
    got_nodes, got_tris = refit_ref.refit(wiped, stale, width, idx, pos)
    refit_ref.diff_report(got_tris, tris, "triangle record (from stale records)")
    refit_ref.diff_report(got_nodes, nodes, "node (from wiped boxes)")


# ---- the bad-vertex rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
def test_bad_vertex_rule_on_a_small_tree(art, host_width, width):
    pos, idx = _soup(64)
    host_width(width)
    nodes, tris, info = hostsim.bvh(art, mesh_scene(art, pos, idx))
    W = width
    new = _shift(pos, 9)
    victims = [5, 40]
    new[3 * 5 + 1, 2] = np.nan; new[3 * 40, 0] = F(-3e18)
    rn, rt = refit_ref.refit(nodes, tris, W, idx, new)
    rn2 = rn.reshape(-1, 8 * W); rt2 = rt.reshape(-1, 12)
    assert np.array_equal(rn2[:, 3::4].view(np.uint32), nodes.reshape(-1, 8 * W)[:, 3::4].view(np.uint32)), "reference / count words changed"
    prim = rt2[:, 9].view(np.int32)
    alive = refit_ref.surviving_records(rn, rt, W)
    lost = np.unique(prim[~alive])
    assert set(victims) <= set(lost.tolist()) and (~alive).sum() <= refit_ref.MAX_LEAF_TRIS * len(victims)
    # a slot is all +inf or all finite; the slots at +inf are exactly the leaf slots holding a victim's record and inner slots above nothing else
    lo = rn2[:, :4 * W].reshape(-1, W, 4)[:, :, :3]; hi = rn2[:, 4 * W:].reshape(-1, W, 4)[:, :, :3]
    ref = rn2[:, 3:4 * W:4].view(np.int32); cnt = rn2[:, 4 * W + 3::4].view(np.int32)
    used = ref >= 0
    inf_slot = np.isposinf(lo).all(2) & np.isposinf(hi).all(2)
    fin_slot = np.isfinite(lo).all(2) & np.isfinite(hi).all(2)
    assert (inf_slot | fin_slot)[used].all()
    for node, j in zip(*np.nonzero(used & (cnt > 0))):
        holds = set(prim[ref[node, j]:ref[node, j] + cnt[node, j]].tolist()) & set(victims)
        assert bool(holds) == bool(inf_slot[node, j])
    # every finite slot bounds exactly the surviving records below it (a plain recursion, no levels): at width 8 its planes ARE the padded
    # min / max of those records' corners, at width 4 they enclose that padded box
    corners = rt2[:, :9].reshape(-1, 3, 3)

    def below(node, j):
        if cnt[node, j] > 0:
            return [r for r in range(ref[node, j], ref[node, j] + cnt[node, j])]
        return [r for k in range(W) if used[ref[node, j], k] and fin_slot[ref[node, j], k] for r in below(ref[node, j], k)]

    for node, j in zip(*np.nonzero(used & fin_slot)):
        recs = below(node, j)
        assert recs and alive[recs].all()
        plo, phi = refit_ref.pad_box(corners[recs].reshape(-1, 3).min(0), corners[recs].reshape(-1, 3).max(0))
        if W == 8:
            assert np.array_equal(lo[node, j].view(np.uint32), plo.view(np.uint32)) and np.array_equal(hi[node, j].view(np.uint32), phi.view(np.uint32))
        else:
            assert (lo[node, j] <= plo).all() and (hi[node, j] >= phi).all()
    for node, j in zip(*np.nonzero(used & inf_slot & (cnt == 0))):                # an inner slot at +inf has nothing alive below it
        assert not any(fin_slot[ref[node, j], k] for k in range(W) if used[ref[node, j], k])


# ---- the shape cases of the GPU test, on the CPU --------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("name", SHAPES)
def test_shape_cases_reference_tree_and_oracle_answer(art, host_width, name, width):
    pos, idx, new = shape_case(name)
    assert np.isfinite(new).all() and np.abs(new).max() <= refit_ref.MAX_COORD
    host_width(width)
    nodes, tris, info = hostsim.bvh(art, mesh_scene(art, pos, idx))
    rn, rt = refit_ref.refit(nodes, tris, width, idx, new)
    assert np.isfinite(rn.reshape(-1, 8 * width)[:, :3]).all()
    bvh_check.check_tree(rn, rt, info["n_nodes"], info["max_stack"], width, new, idx)      # strict enclosure holds in every case: the pad is > 0
    o, d = rays_at(new, idx, 2000, 17)
    want = orc.closest_hits(conv.OracleScene(mesh_scene(art, new, idx)).scene, o, d)
    w = conv.hits_to_arrays(want)
    t, prim, _ = orc.bvh_walk(rn, rt, o, d, width=width)
    hit = w[1] == 1
    if name not in MAY_MISS:
        assert hit.mean() >= 0.25, "only %d of %d rays hit" % (hit.sum(), hit.size)
    assert np.array_equal(prim >= 0, hit), "walk of the reference tree and brute force disagree on is_hit for %d rays" % int(((prim >= 0) != hit).sum())
    assert np.array_equal(prim[hit], w[3][hit])
    if name != "scale_9e17":                                                      # (there the binary32 triangle test overflows: t is not compared)
        assert np.array_equal(t[hit].view(np.uint32), w[0][hit].view(np.uint32))
