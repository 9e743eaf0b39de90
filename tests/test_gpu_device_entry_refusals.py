"""What the device-resident entries of the C ABI refuse, in which order and in which words: the eleven stream-taking entries (the two ray
queries, the two AOV calls, the three denoisers, the two temporal calls, the adaptive estimate, the spatial variance estimate),
art_compact_mask_device and art_render_pass_masked, called through backend.lib (ctypes).  tests/golden/device_entry_refusals.json holds
the return code and the exact art_last_error() text of every case; the test replays the table and compares byte for byte.

    python tests/test_gpu_device_entry_refusals.py --record

writes the JSON from the library as it stands (it needs the GPU).  It was recorded once, from the library as it was before the entries
moved into art_device_entries.cpp and their pointer checks into one list each, and it is not edited by hand: an entry that changes a
refusal on purpose records again and shows the difference in review.

The cases of an entry, over its planes in the order the entry checks them:
  - each plane in turn as a host pointer, and as a device allocation of its own that is one element short (the one-word count_out:
    half a word);
  - order: for every adjacent pair the earlier plane short and the later one on the host -- the earlier one's name is reported,
    although the later one would fail an earlier step of the check; and one bad parameter next to a first plane on the host -- the
    parameter is reported;
  - the unbroken call, accepted.
Every output plane is filled with a sentinel byte and must still hold it after every refused call: nothing was launched.  The frame is
41 x 25 and a query 4097 rays, so that a plane short by one element is a whole number of 4 KiB pages wherever an element is a multiple of
four bytes.  "memory of device N, the library runs on device M" needs two GPUs and is left out.

Beside the table: a query on a side stream that has to grow the scratch while an earlier query is still in flight gives the bits of
the context stream's.  (That a query in several slices with an uneven last one gives the bits of one slice is
tests/test_gpu_ray_queries.py::test_slices_give_the_same_bytes and ::test_queries_between_passes_leave_the_context_alone.)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "device_entry_refusals.json")
F = np.float32
W, H = 41, 25
N = W * H
NRAYS = 4097
SENTINEL = 0xA5


class Entry:
    """planes: [(name as the library reports it, elements, bytes per element, is an output)] in the entry's check order;
    call(pointers by plane name, break a parameter) -> rc; fill: what a good input plane holds instead of zeros"""

    def __init__(self, name, planes, call, fill=None):
        self.name, self.planes, self.call, self.fill = name, planes, call, fill or {}


def run_entry(e, L, hip, got):
    good, host = {}, {}
    for plane, count, per, out in e.planes:
        t = torch.full((count * per,), SENTINEL if out else 0, dtype=torch.uint8, device="cuda")
        if plane in e.fill:
            t.copy_(torch.from_numpy(np.ascontiguousarray(e.fill[plane]).view(np.uint8).reshape(-1)))
        good[plane] = t
        host[plane] = np.zeros(count * per, np.uint8).ctypes       # (a host buffer per plane: two broken planes never overlap)
    outputs = [(plane, good[plane]) for plane, _, _, out in e.planes if out]
    ptrs = {plane: t.data_ptr() for plane, t in good.items()}

    def attempt(case, bad_param=False, first=None, **broken):
        rc = e.call(dict(ptrs, **broken), bad_param)
        text = L.art_last_error().decode() if rc else ""
        torch.cuda.synchronize()
        ident = "%s/%s" % (e.name, case)
        if case != "accepted":
            assert rc != 0, ident
            for plane, t in outputs:
                assert bool((t == SENTINEL).all()), "%s: %s was written" % (ident, plane)
        if first:
            assert text.startswith(first + " is "), (ident, text)
        assert ident not in got
        got[ident] = [rc, text]
        return rc, text

    for i, (plane, count, per, _) in enumerate(e.planes):
        attempt("%s on the host" % plane, first=plane, **{plane: host[plane].data})
        short = C.c_void_p(None)
        assert hip.hipMalloc(C.byref(short), (count - 1) * per if count > 1 else per // 2) == 0
        try:
            attempt("%s one element short" % plane, first=plane, **{plane: short.value})
            if i + 1 < len(e.planes):
                later = e.planes[i + 1][0]
                attempt("order: %s short, %s on the host" % (plane, later), first=plane, **{plane: short.value, later: host[later].data})
        finally:
            hip.hipFree(short)
    plane = e.planes[0][0]
    _, text = attempt("order: a bad parameter, %s on the host" % plane, bad_param=True, **{plane: host[plane].data})
    assert not text.startswith(plane + " is "), (e.name, text)
    rc, text = attempt("accepted")
    assert rc == 0, (e.name, L.art_last_error().decode())


def entries(art, backend, nv, pos):
    """the entries that run on the flat scene (its CLOSEST mesh: nv vertices at pos), then the one that needs two instances"""
    import temporal_ref as T
    L = backend.lib
    n = NRAYS
    i, o = False, True
    rays = [("origins", n, 12, i), ("dirs", n, 12, i), ("tnear", n, 4, i), ("tfar", n, 4, i)]
    ray_fill = {"dirs": np.tile(F([0.0, 0.0, 1.0]), n), "tfar": np.full(n, 1.0e30, F)}
    flat = [Entry("art_trace_rays_device", rays + [("hits_out", n, 44, o)],
                  lambda q, bad: L.art_trace_rays_device(q["origins"], q["dirs"], q["tnear"], q["tfar"], n, q["hits_out"], 7 if bad else art.TRACE_COOP, None), ray_fill),
            Entry("art_occluded_rays_device", rays + [("occluded_out", n, 1, o)],
                  lambda q, bad: L.art_occluded_rays_device(q["origins"], q["dirs"], q["tnear"], q["tfar"], -1 if bad else n, q["occluded_out"], None), ray_fill)]

    aov = [("albedo3f", N, 12, o), ("normal3f", N, 12, o), ("depth", N, 4, o), ("alpha", N, 4, o), ("prim_type", N, 4, o), ("prim_index", N, 4, o), ("mat", N, 4, o)]
    pp = art.Backend.pass_params(art.RT_DEBUG, True, 0, 0, seed=12345, layout=art.LAYOUT_ADA_XY)

    def buf(q):
        return C.byref(art.ArtAovBuffers(*[q[plane] for plane, _, _, _ in aov]))
    flat.append(Entry("art_render_aovs_device", aov, lambda q, bad: L.art_render_aovs_device(None if bad else C.byref(pp), buf(q), None)))
    flat.append(Entry("art_render_aovs_motion_device/flat", [("motion3f", N, 12, o), ("cur_pos3f", nv, 12, i), ("prev_pos3f", nv, 12, i)] + aov,
                      lambda q, bad: L.art_render_aovs_motion_device(C.byref(pp), buf(q), C.byref(art.ArtMotionSource(q["cur_pos3f"], q["prev_pos3f"], nv - 1 if bad else nv, None, 0)),
                                                                     q["motion3f"], None), {"cur_pos3f": pos, "prev_pos3f": pos}))

    guides = [("albedo3f", N, 12, i), ("normal3f", N, 12, i), ("depth", N, 4, i)]
    flat.append(Entry("art_denoise_device", [("color3f", N, 12, i), ("out3f", N, 12, o)] + guides,
                      lambda q, bad: L.art_denoise_device(C.byref(art.ArtDenoiseParams(W, H, 0 if bad else 2, 0, 7, 0, 1.0, 2.0, 1.0)), q["color3f"], q["albedo3f"], q["normal3f"],
                                                          q["depth"], q["out3f"], None)))
    for name, spread, per in (("art_denoise_svgf_device", "moments2f", 8), ("art_denoise_svgf_var_device", "variance1f", 4)):
        def svgf(q, bad, entry=getattr(L, name), spread=spread, plane=(per == 4)):
            p = art.ArtSvgfParams(W, H, 0 if bad and plane else 2, 0, 7, 1 if bad else 2, 1.0, 2.0, 1.0)      # n_colours = 1 | iterations = 0 (the plane's call reads no n_colours)
            return entry(C.byref(p), q["color3f"], q[spread], q["albedo3f"], q["normal3f"], q["depth"], q["out3f"], q["variance_out"], None)
        flat.append(Entry(name, [("color3f", N, 12, i), ("out3f", N, 12, o), (spread, N, per, i)] + guides + [("variance_out", N, 4, o)], svgf))

    def temporal_params(bad):
        p = art.ArtTemporalParams()
        p.cur, p.prev = backend.temporal_camera(T.cam(), W, H), backend.temporal_camera(T.cam((0.1, 0, 0)), W, H)
        p.n_colours, p.max_history, p.scale, p.depth_tol, p.normal_min = 0 if bad else 2, 16, 1.0, 0.05, 0.9
        return C.byref(p)
    temporal = [("color3f", N, 12, i), ("moments2f", N, 8, i), ("hist_out", N, 48, o), ("hist_in", N, 48, i), ("normal3f", N, 12, i), ("depth", N, 4, i), ("id", N, 4, i),
                ("out3f", N, 12, o), ("variance_out", N, 4, o), ("length_out", N, 4, o)]
    for name, moved in (("art_temporal_device", []), ("art_temporal_motion_device", ["motion3f"])):
        def tp(q, bad, entry=getattr(L, name), moved=moved):
            return entry(temporal_params(bad), q["color3f"], q["moments2f"], q["normal3f"], q["depth"], q["id"], *[q[m] for m in moved], q["hist_in"], q["hist_out"],
                         q["out3f"], q["variance_out"], q["length_out"], None)
        flat.append(Entry(name, temporal + [(m, N, 12, i) for m in moved], tp))

    flat.append(Entry("art_adaptive_estimate_device", [("accum3f", N, 12, i), ("moments2f", N, 8, i), ("counts1u", N, 4, i), ("mean3f", N, 12, o), ("variance1f", N, 4, o),
                                                       ("error1f", N, 4, o), ("mask1b", N, 1, o)],
                      lambda q, bad: L.art_adaptive_estimate_device(C.byref(art.ArtAdaptiveParams(W, H, 1, 1 if bad else 2, 1 << 30, 0.05, 0.01)), q["accum3f"], q["moments2f"],
                                                                    q["counts1u"], q["mean3f"], q["variance1f"], q["error1f"], q["mask1b"], None)))
    flat.append(Entry("art_svgf_spatial_variance_device", [("hist", N, 48, i), ("variance_in1f", N, 4, i), ("variance_out1f", N, 4, o)],
                      lambda q, bad: L.art_svgf_spatial_variance_device(C.byref(art.ArtSvgfSpatialParams(W, H, 0 if bad else 1, 7, 4.0, 1.0)), q["hist"], q["variance_in1f"],
                                                                        q["variance_out1f"], None)))
    every = {"mask1b": np.ones(N, np.uint8)}
    flat.append(Entry("art_compact_mask_device", [("mask1b", N, 1, i), ("pixels_out", N, 4, o), ("count_out", 1, 4, o)],
                      lambda q, bad: L.art_compact_mask_device(q["mask1b"], q["pixels_out"], N - 1 if bad else N, q["count_out"], None), every))

    def masked(q, bad):
        p = art.Backend.pass_params(art.PT_MIS, True, 2, 0 if bad else 1, seed=7)
        spp, pixels = C.c_int32(0), C.c_int64(-7)
        rc = L.art_render_pass_masked(C.byref(p), q["mask1b"], q["counts1u"], C.byref(spp), C.byref(pixels))
        assert (spp.value, pixels.value) == ((0, -7) if rc else (4, N))
        return rc
    flat.append(Entry("art_render_pass_masked", [("mask1b", N, 1, i), ("counts1u", N, 4, o)], masked, every))

    one = F([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    two = Entry("art_render_aovs_motion_device/instanced", [("motion3f", N, 12, o), ("prev_m12f", 2, 48, i)] + aov,
                lambda q, bad: L.art_render_aovs_motion_device(C.byref(pp), buf(q), C.byref(art.ArtMotionSource(None, None, 0, q["prev_m12f"], 3 if bad else 2)), q["motion3f"], None),
                {"prev_m12f": np.tile(one, 2)})
    return flat, two


def collect(art, backend):
    """{entry/case: [rc, art_last_error() text]} of the whole table"""
    from ada_ray_tracer_amd import scenes
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    sd = scenes.synthetic_scene(12, 3)                              # Cornell box, three spheres, a CLOSEST soup of 12 triangles
    pos = np.ascontiguousarray(sd._mesh_arrays[-1][0], F)
    flat, two = entries(art, backend, pos.shape[0], pos)
    got = {}
    backend.upload_scene(sd); backend.resize(W, H)
    for e in flat:
        run_entry(e, backend.lib, hip, got)
    backend.upload_scene(scenes.instanced_scene(2, 12)); backend.resize(W, H)
    run_entry(two, backend.lib, hip, got)
    backend.synchronize()
    return got


def test_every_refusal_is_the_recorded_one(art, backend):
    got = collect(art, backend)
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    assert sorted(got) == sorted(want)
    wrong = ["%s: got %r, recorded %r" % (k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "\n".join(wrong)


def test_a_query_that_grows_the_scratch_on_a_side_stream(art, backend):
    """On a non-default stream: a query, a larger one (b_query, b_queue grow while the first may still run: the entry waits for both
    streams first), the first again.  All three hold the bits the context stream gives."""
    import test_gpu_ray_queries as rq
    from ada_ray_tracer_amd import scenes
    sd = scenes.synthetic_scene(12, 3)
    o, d = rq._rays(9001, 17)
    og, dg = rq._gpu(o, d)
    small = 3001
    backend.upload_scene(sd)
    want = backend.trace_rays_torch(og, dg).raw.cpu().numpy()
    want_occ = backend.occluded_torch(og, dg).cpu().numpy()
    assert (want[:, 1] == 1).any() and (want[:, 1] == 0).any()
    backend.shutdown()                                              # the scratch only ever grows: start again without one
    backend.__init__(0)
    backend.upload_scene(sd)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = [(backend.trace_rays_torch(og[:k], dg[:k]).raw, backend.occluded_torch(og[:k], dg[:k])) for k in (small, len(o), small)]
    s.synchronize()
    for hits, occ in got:
        k = hits.shape[0]
        rq._assert_same_bytes(hits, want[:k])
        assert np.array_equal(occ.cpu().numpy(), want_occ[:k])
    backend.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path[:0] = [HERE, os.path.dirname(HERE)]
    import __graft_entry__ as ge
    pkg = ge.load_package()
    be = pkg.Backend(0)
    cases = collect(pkg, be)
    be.shutdown()
    with open(GOLDEN, "w") as f:
        json.dump({"frame": [W, H], "rays": NRAYS, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(cases), GOLDEN))
