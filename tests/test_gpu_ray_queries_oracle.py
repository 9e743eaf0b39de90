"""Device-resident ray queries against the oracle, not against the product: every word of every record of art_trace_rays_device and every
byte of art_occluded_rays_device equals what tests/query_ref.py (the interval rule, written from the headers) makes of the oracle's
O(N) scan of the shifted rays -- on four scenes, both trace kernels, every interval combination, at the exact bound, at the ray counts
where the LDS staging of k_query_pack / k_query_finalize ends inside a workgroup, in slices, and through k_trace_overflow."""
import numpy as np
import pytest

import conv
import hostsim
import orc
import query_ref as Q
from test_gpu_ray_queries import SCENES, _assert_same_bytes, _gpu, _interval_case, _rays, _scene, _shadow_rays_from

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
COMBOS = ["none", "tnear", "tfar", "both"]
# where 3 n, 11 n or n itself crosses a multiple of 256 (k_query_pack stages 3 dwords per ray, k_query_finalize 11, in workgroups of 256)
EDGE_COUNTS = [1, 2, 23, 24, 85, 86, 170, 171, 255, 256, 257, 512, 513]
GUARD_WORDS, PLANTED = 64, 0x5A5A5A5A


class Case:
    """A scene, the oracle's view of it, and one fixed list of rays with the reference records of the four interval combinations
    (computed once per session; nothing below changes them)."""

    def __init__(self, art, name):
        self.name = name
        self.sd, _ = _scene(art, name)
        self.to_product_index = lambda flat: flat
        if name == "reference":
            self._keep = orc.CornellScene()
            self.osc = self._keep.scene
        elif name == "instanced":                                     # the oracle scans the world-space flattening
            d = self.sd.desc
            self._keep = conv.OracleScene(hostsim.flattened_copy(art, self.sd))
            self.osc = self._keep.scene
            ntris = [d.meshes[d.instances[i].mesh].ntris for i in range(d.n_instances)]
            offs = np.concatenate([[0], np.cumsum(ntris)])
            shift = 0
            while (1 << shift) < max(ntris):
                shift += 1

            def to_product_index(flat):                               # position in the flattened list -> instance << shift | triangle of the mesh
                inst = np.searchsorted(offs, flat, side="right") - 1
                return (inst << shift) | (flat - offs[inst])
            self.to_product_index = to_product_index
        else:
            self._keep = conv.OracleScene(self.sd)
            self.osc = self._keep.scene
        assert self.osc.n_meshes == 1                                 # (a triangle index names a triangle of THE mesh)
        m = self.osc.meshes[0]
        self.pos = np.ctypeslib.as_array(m.pos, (m.nverts, 3)).copy()
        self.idx = np.ctypeslib.as_array(m.idx, (m.ntris, 3)).copy()

        n = 5000 if name == "instanced" else 20000
        o, d = _rays(n, 11)
        first = self.scan(o, d)
        self.surface = first[:, Q.IS_HIT] == 1                        # (of the rays before the restart: the shadow rays start there)
        self.surface_p = (o[self.surface] + first[self.surface, Q.T].view(F)[:, None] * d[self.surface]).astype(F)
        restart = np.nonzero(self.surface)[0][::2]                    # half of the hitting rays start on the surface they hit, by the oracle's t
        o = o.copy()
        o[restart] = o[restart] + first[restart, Q.T].view(F)[:, None] * d[restart]
        self.o, self.d = np.ascontiguousarray(o), d
        self.tn, self.tf = _interval_case(n, 5)
        self.args = {"none": (None, None), "tnear": (self.tn, None), "tfar": (None, self.tf), "both": (self.tn, self.tf)}
        self.scan_plain = self.scan(self.o, self.d)
        self.scan_shifted = self.scan(Q.shifted(self.o, self.d, self.tn)[0], self.d)
        self.want, self.occluded = {}, {}
        for c, (tn, tf) in self.args.items():
            self.want[c], self.occluded[c] = Q.records(self.o, self.d, tn, tf, self.scan_plain if tn is None else self.scan_shifted)
            self.want[c].setflags(write=False); self.occluded[c].setflags(write=False)
        # the mix the cases are about: hits and misses everywhere, empty intervals and hits cut off by the bound with tfar
        for c in COMBOS:
            assert self.occluded[c].sum() > n // 10 and (~self.occluded[c]).sum() > n // 10, (name, c)
        live = Q.shifted(self.o, self.d, self.tn, self.tf)[3]
        assert (~live).sum() > n // 20 and (live & ~self.occluded["both"] & (self.scan_shifted[:, Q.IS_HIT] == 1)).sum() > n // 20
        self.triangle_hits = int((self.scan_plain[:, Q.PRIM_TYPE][self.scan_plain[:, Q.IS_HIT] == 1] == Q.PRIM_TRIANGLE).sum())
        assert self.triangle_hits > (20 if name == "reference" else n // 50), self.triangle_hits      # (the reference's pyramid is small)

    def scan(self, o, d):
        """the oracle's closest hits of the rays as query_ref takes them: barycentrics in words 9, 10, the product's triangle numbering"""
        o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
        w = np.frombuffer(orc.closest_hits(self.osc, o, d), np.int32).reshape(-1, Q.WORDS).copy()
        tri = np.nonzero((w[:, Q.IS_HIT] == 1) & (w[:, Q.PRIM_TYPE] == Q.PRIM_TRIANGLE))[0]
        u, v = np.zeros(len(o), F), np.zeros(len(o), F)
        corners = self.idx[w[tri, Q.PRIM_INDEX]]
        t, u[tri], v[tri] = Q.barycentrics(o[tri], d[tri], self.pos[corners[:, 0]], self.pos[corners[:, 1]], self.pos[corners[:, 2]])
        assert np.array_equal(t.view(np.int32), w[tri, Q.T])          # the triangle the oracle names, by its own arithmetic: its t to the bit
        w[tri, Q.PRIM_INDEX] = self.to_product_index(w[tri, Q.PRIM_INDEX])
        return Q.scan_records(w, u, v)

    def gpu(self, combo, n=None):
        tn, tf = self.args[combo]
        cut = lambda a: None if a is None else a[:n]
        return _gpu(self.o[:n], self.d[:n], cut(tn), cut(tf))

    def host(self, combo, n=None):
        tn, tf = self.args[combo]
        cut = lambda a: None if a is None else a[:n]
        return [self.o[:n], self.d[:n], cut(tn), cut(tf)]


_cases = {}


def case(art, name):
    if name not in _cases:
        _cases[name] = Case(art, name)
    return _cases[name]


def _kernels(art):
    return {"coop": art.TRACE_COOP, "simple": art.TRACE_SIMPLE}


def _assert_inputs_kept(tensors, arrays):
    """(e) the caller's tensors hold the bytes they were given"""
    for name, t, a in zip(("origins", "dirs", "tnear", "tfar"), tensors, arrays):
        if t is not None:
            assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(a, F).view(np.uint32)), name + " was written by the query"


# ---- (a) closest hit: all 11 words of every record ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["coop", "simple"])
@pytest.mark.parametrize("scene", SCENES)
def test_closest_hit_records_equal_the_oracle_under_the_interval_rule(art, backend, scene, kernel):
    c = case(art, scene)
    backend.upload_scene(c.sd)
    for combo in COMBOS:
        args = c.gpu(combo)
        got = backend.trace_rays_torch(*args, kernel=_kernels(art)[kernel])
        _assert_same_bytes(got.raw, c.want[combo])
        _assert_inputs_kept(args, c.host(combo))


# ---- (b) occlusion: the shadow rule's early exit against the same reference --------------------------------------------------------------
def _shadow_case(c):
    """surface points (the oracle's hits) towards light samples, tnear = 1e-4, tfar = 0.999 dist; and what the oracle says of them"""
    if not hasattr(c, "shadow"):
        p, sdir, tn, tf = _shadow_rays_from(c.sd, c.surface_p, np.random.default_rng(37))
        want, occ = Q.records(p, sdir, tn, tf, c.scan(Q.shifted(p, sdir, tn)[0], sdir))
        assert occ.any() and not occ.all(), occ.mean()                # both answers occur
        c.shadow = (p, sdir, tn, tf, want, occ)
    return c.shadow


@pytest.mark.parametrize("stack", ["tree_bound", "lds_stack_cap_3"])
@pytest.mark.parametrize("scene", SCENES)
def test_occlusion_equals_the_oracle_under_the_interval_rule(art, backend, scene, stack):
    """art_occluded_rays_device takes no kernel argument (it runs the cooperative kernel); lds_stack_cap = 3 sends the rays whose stack
    does not fit through k_trace_overflow, with the shadow rule"""
    c = case(art, scene)
    p, sdir, stn, stf, swant, socc = _shadow_case(c)
    backend.set_option("lds_stack_cap", 3 if stack == "lds_stack_cap_3" else 0)
    try:
        backend.upload_scene(c.sd)
        if stack == "lds_stack_cap_3" and scene in ("synthetic", "rect"):
            assert backend.bvh_info().max_stack > 3                    # the cap is below the tree's bound: the checked-push kernel runs
        for combo in COMBOS:
            args = c.gpu(combo)
            got = backend.occluded_torch(*args).cpu().numpy()
            assert got.dtype == np.bool_
            bad = np.nonzero(got != c.occluded[combo])[0]
            assert bad.size == 0, "%s: %d of %d rays differ, first %d: got %s" % (combo, bad.size, len(got), bad[0], got[bad[0]])
            _assert_inputs_kept(args, c.host(combo))
        args = _gpu(p, sdir, stn, stf)
        got = backend.occluded_torch(*args).cpu().numpy()
        bad = np.nonzero(got != socc)[0]
        assert bad.size == 0, "shadow rays: %d of %d differ, first %d: got %s" % (bad.size, len(got), bad[0], got[bad[0]])
        _assert_same_bytes(backend.trace_rays_torch(*args).raw, swant)    # (and the closest hit of the same rays, through the same stack plan)
        _assert_inputs_kept(args, [p, sdir, stn, stf])
    finally:
        backend.set_option("lds_stack_cap", 0)


# ---- (c) the exact bound ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
def test_a_hit_at_tfar_is_a_miss_and_one_ulp_inside_it_a_hit(art, backend, scene):
    """2000 hitting rays, no tnear: tfar = the oracle's t to the bit (even rays) and the next float above it (odd rays), side by side
    in one call, so the lanes of one wave fall on both sides of the bound"""
    c = case(art, scene)
    backend.upload_scene(c.sd)
    sel = np.nonzero(c.scan_plain[:, Q.IS_HIT] == 1)[0][:2000]
    assert len(sel) == 2000
    o, d, scan = np.ascontiguousarray(c.o[sel]), np.ascontiguousarray(c.d[sel]), c.scan_plain[sel]
    t = scan[:, Q.T].view(F)
    tfar = t.copy()
    tfar[1::2] = np.nextafter(t[1::2], F(np.inf))
    unbounded, _ = Q.records(o, d, None, None, scan)
    want, occ = Q.records(o, d, None, tfar, scan)
    def at_and_above_the_bound(rec, who):
        """at the bound a miss that holds tfar, one ulp above it the record of the unbounded query"""
        assert not rec[0::2, Q.IS_HIT].any() and np.array_equal(rec[0::2, Q.T], tfar[0::2].view(np.int32)), who
        assert (rec[0::2, Q.PRIM_TYPE:Q.MAT + 1] == -1).all() and not rec[0::2, Q.NX:].any(), who
        assert np.array_equal(rec[1::2], unbounded[1::2]) and rec[1::2, Q.IS_HIT].all(), who

    at_and_above_the_bound(want, "query_ref")                          # (the rule says so itself)
    assert np.array_equal(occ, np.arange(2000) % 2 == 1)
    args = _gpu(o, d, None, tfar)
    for name, k in _kernels(art).items():
        got = backend.trace_rays_torch(*args, kernel=k).raw.cpu().numpy()
        _assert_same_bytes(got, want)
        at_and_above_the_bound(got, name)
    assert np.array_equal(backend.occluded_torch(*args).cpu().numpy(), occ)
    _assert_inputs_kept(args, (o, d, None, tfar))


# ---- (d) ray counts at the staging edges ----------------------------------------------------------------------------------------------
def _stream(art):
    return torch.cuda.current_stream().cuda_stream or art.HIP_STREAM_LEGACY


@pytest.mark.parametrize("kernel", ["coop", "simple"])
def test_ray_counts_where_the_lds_staging_ends_inside_a_workgroup(art, backend, kernel):
    """The first n of one list of rays through the C ABI into a tensor with planted words after record n (and planted bytes after byte
    n of the occlusion answer): the first n reference records, and not a word behind them."""
    c = case(art, "synthetic")
    backend.upload_scene(c.sd)
    L = backend.lib
    nmax = max(EDGE_COUNTS)
    og, dg, tng, tfg = c.gpu("both", nmax)
    for n in EDGE_COUNTS:
        out = torch.full((n * Q.WORDS + GUARD_WORDS,), PLANTED, dtype=torch.int32, device="cuda")
        assert L.art_trace_rays_device(og.data_ptr(), dg.data_ptr(), tng.data_ptr(), tfg.data_ptr(), n, out.data_ptr(), _kernels(art)[kernel], _stream(art)) == 0, L.art_last_error()
        got = out.cpu().numpy()
        _assert_same_bytes(got[:n * Q.WORDS].reshape(n, Q.WORDS), c.want["both"][:n])
        assert (got[n * Q.WORDS:] == PLANTED).all(), "n = %d: words behind record n were written" % n
    if kernel == "coop":                                              # (the occlusion entry has one kernel)
        for n in EDGE_COUNTS:
            occ = torch.full((n + GUARD_WORDS,), 0x5A, dtype=torch.uint8, device="cuda")
            assert L.art_occluded_rays_device(og.data_ptr(), dg.data_ptr(), tng.data_ptr(), tfg.data_ptr(), n, occ.data_ptr(), _stream(art)) == 0, L.art_last_error()
            got = occ.cpu().numpy()
            assert np.array_equal(got[:n], c.occluded["both"][:n].astype(np.uint8)) and (got[n:] == 0x5A).all(), n
    _assert_inputs_kept((og, dg, tng, tfg), c.host("both", nmax))


@pytest.mark.parametrize("kernel", ["coop", "simple"])
def test_slices_that_end_at_the_staging_edges(art, backend, kernel):
    """513 rays in slices of 1, 255, 256 and 257: the bytes of the unsliced call, which are the reference's"""
    c = case(art, "synthetic")
    backend.upload_scene(c.sd)
    n, k = 513, _kernels(art)[kernel]
    args = c.gpu("both", n)
    want = c.want["both"][:n]
    whole = backend.trace_rays_torch(*args, kernel=k).raw.cpu().numpy()
    _assert_same_bytes(whole, want)
    try:
        for s in (1, 255, 256, 257):
            backend.set_option("query_slice", s)
            got = backend.trace_rays_torch(*args, kernel=k).raw.cpu().numpy()
            _assert_same_bytes(got, whole)
            _assert_same_bytes(got, want)
            if kernel == "coop":
                assert np.array_equal(backend.occluded_torch(*args).cpu().numpy(), c.occluded["both"][:n]), s
    finally:
        backend.set_option("query_slice", 1 << 24)
    _assert_inputs_kept(args, c.host("both", n))


# ---- (e) inputs as given --------------------------------------------------------------------------------------------------------------
def test_the_callers_tensors_keep_their_bytes(art, backend):
    """Origins with -0 components under tnear = 0 and under no tnear, among rays that are shifted: a pack stage that shifted in place
    would leave +0 (o + 0 * d) or the shifted origin behind.  Every call of the tests above is checked in the same way."""
    c = case(art, "synthetic")
    backend.upload_scene(c.sd)
    n = 1000
    o, d, tn, tf = (a.copy() for a in c.host("both", n))
    o[::3] = np.where(np.abs(o[::3]) < 1.0, F(-0.0), o[::3])
    o[1::3, 0] = F(-0.0)
    tn[::2] = 0.0
    assert np.signbit(o).any() and (tn > 0).any()
    for tnear, tfar in ((None, None), (tn, None), (None, tf), (tn, tf)):
        args = _gpu(o, d, tnear, tfar)
        scan = c.scan(Q.shifted(o, d, tnear)[0], d)
        want, occ = Q.records(o, d, tnear, tfar, scan)
        for k in _kernels(art).values():
            _assert_same_bytes(backend.trace_rays_torch(*args, kernel=k).raw, want)
            _assert_inputs_kept(args, (o, d, tnear, tfar))
        assert np.array_equal(backend.occluded_torch(*args).cpu().numpy(), occ)
        _assert_inputs_kept(args, (o, d, tnear, tfar))
