"""Null shadow rays -- shadow rays whose explicit colour is exactly zero whatever their verdict (the light sample behind the surface,
or a BxDF of zero) -- in the record schedule's default pass: not walked, still counted (DevFrame::skip_null_shadow = kNullShadowCounted).

The comparators walk every shadow ray: the counting variant (count_tests = 1) and the one-ray-per-lane schedule (trace_kernel = simple).
Against each of them the default pass must give the same accum bits, the same ArtStats::rays (the reference's Find_Closest_Hit /
Compute_Shadow calls) and lose no path.  A scene without null candidates would make all of this vacuous, so every case also renders
with option skip_null_shadow = 1 (not walked, NOT counted) and asserts that it counts fewer rays than the default.

160 x 120, AA on, 2 vthreads (8 spp), seed 13.  Cases: PT_MIS at depth 8 on the option test's three scenes and on the rect-light scene
whose candidates overflow to NaN on the ceiling (NaN compares unequal to zero: still traced); PT_MIS at depth 1, where the only stage
writes a REC_SHADOW bank in which an item's only record may be absent; PT_SHADOW at depth 8 (shade_item's other candidate expression).
An instanced scene renders through the record schedule only, so it has no trace_kernel = simple leg.  Every (scene, case) is uploaded
and rendered once, leg by leg, and the tests share the results."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 160, 120

SCENES = {
    "c3_small": lambda scenes: scenes.synthetic_scene(20000, 3),
    "mixed": lambda scenes: scenes.mixed_scene(5000, 5),
    "instanced": lambda scenes: scenes.instanced_scene(12, 300),
    "rect_nan": lambda scenes: scenes.synthetic_scene(2000, 3, rect_lights=True),
}
# (scene, render type, max_depth)
CASES = [("c3_small", "PT_MIS", 8), ("mixed", "PT_MIS", 8), ("instanced", "PT_MIS", 8), ("rect_nan", "PT_MIS", 8),
         ("c3_small", "PT_MIS", 1), ("c3_small", "PT_SHADOW", 8)]
# leg -> the options it sets (all back to their defaults afterwards)
LEGS = {"default": {}, "count_tests": {"count_tests": 1}, "simple": {"trace_kernel": 1}, "skip": {"skip_null_shadow": 1}}
DEFAULTS = {"count_tests": 0, "trace_kernel": 0, "skip_null_shadow": 0}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def has_leg(scene, leg):
    return not (scene == "instanced" and leg == "simple")


_uploaded = [None]
_results = {}


def legs_of(art, backend, scene, rt, depth):
    """{leg: (accum bits, rays of the pass, lost_paths after it)} of one case, rendered once"""
    key = (scene, rt, depth)
    if key in _results:
        return _results[key]
    from ada_ray_tracer_amd import scenes
    if _uploaded[0] != scene:
        _uploaded[0] = None
        backend.upload_scene(SCENES[scene](scenes))
        _uploaded[0] = scene
    p = art.Backend.pass_params(getattr(art, rt), True, depth, 2, seed=13)
    out = {}
    for leg, options in LEGS.items():
        if not has_leg(scene, leg):
            continue
        for name, value in options.items():
            backend.set_option(name, value)
        try:
            backend.resize(W, H)                          # (a fresh frame; zeroes the counters)
            r0 = backend.stats().rays
            accum, _, spp = backend.render_pass(p, 0)
            st = backend.stats()
        finally:
            for name in options:
                backend.set_option(name, DEFAULTS[name])
        assert spp == 8
        out[leg] = (bits(accum).copy(), st.rays - r0, st.lost_paths)
    _results[key] = out
    return out


@pytest.fixture(scope="module", autouse=True)
def _forget_the_upload_of_another_module():
    _uploaded[0] = None
    yield
    _results.clear()


@pytest.mark.parametrize("scene,rt,depth,walker", [c + (w,) for c in CASES for w in ("count_tests", "simple") if has_leg(c[0], w)])
def test_default_pass_equals_the_pass_that_walks_every_shadow_ray(art, backend, scene, rt, depth, walker):
    legs = legs_of(art, backend, scene, rt, depth)
    got, rays, lost = legs["default"]
    ref, rays_ref, lost_ref = legs[walker]
    print("%s %s depth %d: rays default %d, %s %d, skip_null_shadow=1 %d" % (scene, rt, depth, rays, walker, rays_ref, legs["skip"][1]))
    assert np.array_equal(got, ref)
    assert rays == rays_ref
    assert lost == 0 and lost_ref == 0


@pytest.mark.parametrize("scene,rt,depth", CASES)
def test_the_case_has_null_shadow_rays(art, backend, scene, rt, depth):
    """not vacuous: the option that does not count them counts fewer rays than the default, which counts them -- and gives the same frame"""
    legs = legs_of(art, backend, scene, rt, depth)
    assert 0 < legs["skip"][1] < legs["default"][1]
    assert np.array_equal(legs["skip"][0], legs["default"][0]) and legs["skip"][2] == 0
