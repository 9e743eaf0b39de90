"""art_adaptive_estimate_device without a GPU: tests/adaptive_host, a stand-alone g++ build (AddressSanitizer, UBSan) of the product's own
csrc/art_adaptive.h run as a process of its own, is held bit for bit to tests/adaptive_ref.py, the numpy reference written from the header
text.  The planted planes (adaptive_ref.planted) cover s = 0, n = 1, D < 0, NaN and infinite moments and accum, s at and above
max_samples, an error exactly equal to the threshold, and both values of aa_on."""
import os
import struct
import subprocess

import numpy as np
import pytest

import adaptive_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
PROG = os.path.join(HERE, "adaptive_host", "adaptive_host")
F = np.float32


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(PROG)])
    return PROG


def run_host(prog, tmp_path, accum, moments, counts, aa_on, min_colours, max_samples, threshold, lum_floor):
    H, W = counts.shape
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<5i2f", W, H, int(aa_on), min_colours, max_samples, threshold, lum_floor))
        f.write(np.ascontiguousarray(accum, F).tobytes()); f.write(np.ascontiguousarray(moments, F).tobytes())
        f.write(np.ascontiguousarray(counts, np.uint32).tobytes())
    r = subprocess.run([prog, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]          # (a sanitizer report ends the program with a status of its own)
    raw = open(dst, "rb").read()
    N = W * H
    assert len(raw) == 21 * N
    mean = np.frombuffer(raw, F, 3 * N).reshape(H, W, 3)
    var = np.frombuffer(raw, F, N, 12 * N).reshape(H, W)
    err = np.frombuffer(raw, F, N, 16 * N).reshape(H, W)
    mask = np.frombuffer(raw, np.uint8, N, 20 * N).reshape(H, W)
    return mean, var, err, mask


def same_words(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_the_programs_own_checks(prog):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "adaptive_host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("lum_floor", [0.0, 0.01])
@pytest.mark.parametrize("aa_on", [False, True], ids=["noaa", "aa"])
def test_planted_planes(prog, tmp_path, aa_on, lum_floor):
    W, H, max_samples, min_colours = 70, 50, 96, 4
    accum, mom, counts, thr = R.planted(W, H, aa_on, max_samples, lum_floor)
    want = R.estimate(accum, mom, counts, aa_on, min_colours, max_samples, thr, lum_floor)
    got = run_host(prog, tmp_path, accum, mom, counts, aa_on, min_colours, max_samples, float(thr), lum_floor)
    for name, g, w in zip(("mean", "variance", "error"), got, want):
        assert same_words(g, w), "%s: %d words differ" % (name, int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).sum()))
    assert np.array_equal(got[3], want[3])
    # what the planted pixels must show, stated here and not taken from either side
    mean, var, err, mask = (x.reshape(-1, *x.shape[2:]) for x in got)
    inf = F(np.inf)
    assert not mean[0].any() and not np.signbit(mean[0]).any() and var[0] == inf and err[0] == inf and mask[0] == 1      # s = 0
    assert var[1] == inf and err[1] == inf and mask[1] == 1 and mean[1].any()                                          # n = 1
    assert var[2] == 0 and err[2] == 0 and mask[2] == 1                                                                # D < 0: clamped; 2 colours < min_colours
    assert np.isnan(err[3]) and np.isnan(err[4]) and mask[3] == 1 and mask[4] == 1                                     # NaN moments keep selecting
    assert np.isnan(mean[7][0]) and mean[7][1] == inf and mean[7][2] == -inf
    assert np.signbit(mean[8][0]) and not np.signbit(mean[8][1])                                                       # -0 stays -0
    assert mask[9] == 0 and mask[10] == 0 and mask[12] == 1                                                            # at, above and below max_samples
    assert err[11] == thr and mask[11] == 0                                                                            # an error equal to the threshold is converged
    assert (mask[17:] == 1).any() and (mask[17:] == 0).any()


def test_threshold_one_ulp_below_selects(prog, tmp_path):
    W, H, max_samples = 70, 50, 96
    accum, mom, counts, thr = R.planted(W, H, True, max_samples, 0.01)
    below = float(np.nextafter(thr, F(0.0)))
    got = run_host(prog, tmp_path, accum, mom, counts, True, 2, max_samples, below, 0.01)
    assert got[3].reshape(-1)[11] == 1 and np.array_equal(got[3], R.estimate(accum, mom, counts, True, 2, max_samples, below, 0.01)[3])


def test_zero_counts_select_every_pixel(prog, tmp_path):
    z = np.zeros((5, 7), np.uint32)
    got = run_host(prog, tmp_path, np.ones((5, 7, 3), F), np.ones((5, 7, 2), F), z, True, 2, 8, 0.05, 0.01)
    assert got[3].all() and not got[0].any() and np.isinf(got[1]).all()
    assert np.array_equal(got[3], R.estimate(np.ones((5, 7, 3), F), np.ones((5, 7, 2), F), z, True, 2, 8, 0.05, 0.01)[3])


def test_compaction_statement():
    """the numpy statement of the compaction the GPU test uses: list order is kept, the count is the mask's population over the list"""
    import pixmap_ref
    W, H = 70, 50
    own = pixmap_ref.owner_mask(W, H, 1, 3, 32)
    pixmap = np.flatnonzero(own.reshape(-1)).astype(np.uint32)[::-1].copy()      # any order of the list: the statement keeps it
    rng = np.random.default_rng(3)
    mask = (rng.random((H, W)) < 0.3).astype(np.uint8) * 7
    out = R.compact(mask, pixmap)
    assert len(out) == int((mask != 0)[own].sum()) and np.all(np.diff(out.astype(np.int64)) < 0) and mask.reshape(-1)[out].all()
