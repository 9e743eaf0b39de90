"""art_temporal_upsample_device without a GPU: the product's text (csrc/art_temporal_upsample.h) compiled by g++ with AddressSanitizer and
UBSan as a stand-alone program (tests/temporal_upsample_host) against the numpy reference written from the header
(tests/temporal_upsample_ref.py), bit for bit on every history word, output word and fallback byte; the five lines of step C are all
visited; and the anchor: at lo size == hi size and jitter 0 the new reference IS tests/temporal_ref.py (with a motion plane
tests/temporal_motion_ref.py), for every legal radius."""
import subprocess

import numpy as np
import pytest

import temporal_motion_ref as TM
import temporal_ref as T
import temporal_upsample_ref as R


def test_host_program_passes_its_own_checks():
    out = subprocess.check_output([R.host_program()], text=True)
    assert out.strip() == "temporal_upsample_host: ok"


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_host_build_equals_the_reference(shape):
    res = R.reference_results(shape)
    host = R.temporal_upsample_host_many([kw for _, kw, _ in res])
    wrong = []
    for (name, kw, ref), got in zip(res, host):
        d = [R.differ(a, b) for a, b in zip(ref[:5], got)]
        if any(d):
            wrong.append("%s: words that differ in (hist_out, out3f, variance, length), bytes in fallback: %s" % (name, d))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[2] * s[3] >= 12], ids=R.SHAPE_IDS)
def test_the_reference_visits_every_line_of_step_c(shape):
    """so that no case above can pass by leaving a line out"""
    res = dict((name, r) for name, _, r in R.reference_results(shape))
    branch, fb = res["five_branches"][5], res["five_branches"][4]
    assert sorted(np.unique(branch)) == [0, 1, 2, 3, 4], np.bincount(branch.ravel(), minlength=5)
    assert ((fb == 1) == (branch == 3)).all() and ((fb == 2) == (branch == 4)).all()
    n = res["five_branches"][3]
    assert (n[branch == 4] == 0).all() and (n[branch != 4] > 0).all()


def test_lo_samples_land_where_the_jittered_grid_puts_them():
    """a property the bit comparisons do not state: a jitter of (jx, jy) lo pixels moves the sample under the hi pixel by that much; at a
    ratio of 2 and a jitter of (0.25, 0.25) the lo sample (i, j) lies exactly on the centre of hi pixel (2 i + 1, 2 j + 1): that pixel takes
    it whole (K = 1, length n_cur), its neighbours take less"""
    LW = LH = 4
    rng = np.random.default_rng(3)
    lc = rng.uniform(0.5, 2.0, (LH, LW, 3)).astype(R.F)
    lm = rng.uniform(0.5, 2.0, (LH, LW, 2)).astype(R.F)
    hist, out, var, n, fb = R.temporal_upsample(lc, lm, 4, T.cam(), size=(8, 8), jitter=(0.25, 0.25), radius=1.0, scale=1.0)
    assert (out[1::2, 1::2] == lc).all() and (n[1::2, 1::2] == 4).all()
    assert (n[0::2, 0::2] == 1).all() and (fb == 0).all()              # 0.25 * n_cur = min_confidence * n_cur: a corner between four samples


# ---- the anchor ---------------------------------------------------------------------------------------------------------------------
def finite_case(kw):
    arrs = [kw[k] for k in ("color", "moments", "normal", "depth", "hist", "motion") if kw.get(k) is not None]
    return all(np.isfinite(a).all() for a in arrs)


def as_upsample(kw, radius, min_confidence):
    """temporal_ref's keyword arguments as temporal_upsample's, with the one frame on both sides"""
    g = dict(normal=kw.get("normal"), depth=kw.get("depth"), id=kw.get("ids"))
    hi = dict(g, motion=kw.get("motion"))
    H, W = kw["color"].shape[:2]
    return dict(lo_color=kw["color"], lo_moments=kw["moments"], n_colours=kw["n_colours"], cam_cur=kw["cam_cur"], cam_prev=kw["cam_prev"], hist=kw["hist"], lo=g, hi=hi,
                size=(W, H), jitter=(0.0, 0.0), radius=radius, min_confidence=min_confidence, max_history=kw["max_history"], depth_tol=kw["depth_tol"],
                normal_min=kw["normal_min"], scale=kw["scale"])


def own_tap_counts(kw):
    """the anchor's other condition: every pixel passes its own tests -- a miss (depth 0) is told from a hit by the depth plane, and
    without it a miss's zero normal fails dot(N, N) >= normal_min"""
    return kw.get("depth") is not None or kw.get("normal") is None


@pytest.mark.parametrize("size", [(13, 9), (64, 33)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("radius", [1.0, 0.37, 2.0 ** -20])
def test_at_equal_sizes_and_jitter_0_the_reference_is_temporal_ref(size, radius):
    ran = 0
    for name, kw in T.cases(*size):
        if not (finite_case(kw) and own_tap_counts(kw)):
            continue
        want = T.temporal(**kw)
        got = R.temporal_upsample(**as_upsample(kw, radius, 0.25))
        d = [R.differ(a, b) for a, b in zip(want, got[:4])]
        assert not any(d) and not got[4].any(), (name, d)
        ran += 1
    assert ran >= 12


@pytest.mark.parametrize("radius", [1.0, 0.5])
def test_at_equal_sizes_and_jitter_0_with_motion_the_reference_is_temporal_motion_ref(radius):
    ran = 0
    for name, kw in TM.cases(13, 9):
        if not (finite_case(kw) and own_tap_counts(kw)):
            continue
        want = TM.temporal(**kw)
        got = R.temporal_upsample(**as_upsample(kw, radius, 0.25))
        d = [R.differ(a, b) for a, b in zip(want, got[:4])]
        assert not any(d) and not got[4].any(), (name, d)
        ran += 1
    assert ran >= 8


def test_the_anchor_through_the_host_build():
    """the same through the g++ build of the product's text, held to the g++ build of art_temporal.h's (tests/temporal_ref.temporal_host is
    loaded into python and is not used here: the reference above stands for it)"""
    calls, wants = [], []
    for name, kw in T.cases(13, 9) + TM.cases(13, 9):
        if finite_case(kw) and own_tap_counts(kw):
            calls.append(as_upsample(kw, 1.0, 0.25))
            wants.append(TM.temporal(**kw))
    for want, got in zip(wants, R.temporal_upsample_host_many(calls)):
        assert not any(R.differ(a, b) for a, b in zip(want, got[:4])) and not got[4].any()
