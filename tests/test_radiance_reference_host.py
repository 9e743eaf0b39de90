"""art_radiance_rays_device without a GPU: tests/radiance_host, a stand-alone g++ build of the product's own csrc/art_radiance.h (plain, and
with AddressSanitizer + UBSan), run as processes of their own and held bit for bit to tests/radiance_ref.py, the numpy reference written
from the header text: the association of the radiance and moment sums (1, 3, 8 samples; two calls against one; any cut into sample
batches; non-finite path values), and every hot word raygen leaves for a ray (1, 63, 64, 65, 257 rays)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import radiance_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "radiance_host")
F = np.float32


@pytest.fixture(scope="module", params=["radiance_host", "radiance_host_san"])
def prog(request):
    subprocess.check_call(["make", "-s", "-C", DIR, request.param])
    return os.path.join(DIR, request.param)


def run(prog, tmp_path, header, arrays, tag):
    src, dst = tmp_path / ("in_%s.bin" % tag), tmp_path / ("out_%s.bin" % tag)
    with open(src, "wb") as f:
        f.write(struct.pack("<5i", *header))
        for a in arrays:
            f.write(np.ascontiguousarray(a, F).tobytes())
    r = subprocess.run([prog, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]          # (a sanitizer report ends the program with a status of its own)
    return open(dst, "rb").read()


def host_accumulate(prog, tmp_path, values, radiance, moments, chunk, with_moments=True, tag="a"):
    n, samples = values.shape[:2]
    raw = run(prog, tmp_path, (0, n, samples, chunk, int(with_moments)), [values, radiance, moments], tag)
    assert len(raw) == 20 * n
    return np.frombuffer(raw, F, 3 * n).reshape(n, 3), np.frombuffer(raw, F, 2 * n, 12 * n).reshape(n, 2)


def words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def path_values(n, samples, seed):
    """path values as a render produces them: mostly small, some exact zeros (misses), some large (a light seen directly), widely
    different magnitudes within a ray so that the order of the additions shows in the last bits"""
    rng = np.random.default_rng(seed)
    v = (rng.random((n, samples, 3)) * np.exp(rng.uniform(-12, 4, (n, samples, 1)))).astype(F)
    v[rng.random((n, samples)) < 0.2] = 0.0
    return v


def test_the_programs_own_checks(prog):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "radiance_host: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("samples", [1, 3, 8])
def test_sums_have_the_headers_association(prog, tmp_path, samples):
    n = 257
    v = path_values(n, samples, 100 + samples)
    rng = np.random.default_rng(7)
    rad0 = rng.random((n, 3)).astype(F); mom0 = rng.random((n, 2)).astype(F)      # read-modify-write: the planes hold something
    want_r, want_m = R.accumulate(v, rad0, mom0)
    for chunk in sorted({1, 2, samples}):                                         # however the samples are cut into batches
        got_r, got_m = host_accumulate(prog, tmp_path, v, rad0, mom0, chunk, tag="c%d" % chunk)
        assert np.array_equal(words(got_r), words(want_r)) and np.array_equal(words(got_m), words(want_m)), (samples, chunk)
    # the order matters at this data: the sums taken the other way round differ, so an implementation that reordered them would show
    rev_r, _ = R.accumulate(v[:, ::-1], rad0, mom0)
    assert samples == 1 or not np.array_equal(words(rev_r), words(want_r))
    # without moments the plane is left alone and the radiance is the same
    got_r, got_m = host_accumulate(prog, tmp_path, v, rad0, mom0, samples, with_moments=False, tag="nomom")
    assert np.array_equal(words(got_r), words(want_r)) and np.array_equal(words(got_m), words(mom0))


def test_two_calls_equal_one(prog, tmp_path):
    n = 65
    v = path_values(n, 8, 5)
    zero3, zero2 = np.zeros((n, 3), F), np.zeros((n, 2), F)
    one_r, one_m = host_accumulate(prog, tmp_path, v, zero3, zero2, 8, tag="one")
    a_r, a_m = host_accumulate(prog, tmp_path, v[:, :4], zero3, zero2, 4, tag="first")
    b_r, b_m = host_accumulate(prog, tmp_path, v[:, 4:], a_r, a_m, 4, tag="second")
    assert np.array_equal(words(b_r), words(one_r)) and np.array_equal(words(b_m), words(one_m))
    want_r, want_m = R.accumulate(v)
    assert np.array_equal(words(one_r), words(want_r)) and np.array_equal(words(one_m), words(want_m))


def test_non_finite_path_values(prog, tmp_path):
    n, samples = 8, 3
    v = path_values(n, samples, 9)
    v[0, 1, 0] = np.nan; v[1, 0, 1] = np.inf; v[2, 2, 2] = -np.inf; v[3, 0] = np.inf; v[3, 1] = -np.inf      # inf - inf: NaN in every sum
    v[4, 1] = F(3.0e38); v[4, 2] = F(3.0e38)                                                                   # overflow of the sums themselves
    zero3, zero2 = np.zeros((n, 3), F), np.zeros((n, 2), F)
    got_r, got_m = host_accumulate(prog, tmp_path, v, zero3, zero2, samples)
    want_r, want_m = R.accumulate(v)
    for g, w in ((got_r, want_r), (got_m, want_m)):
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(words(g)[~np.isnan(g)], words(w)[~np.isnan(w)])
    assert np.isnan(got_r[0, 0]) and np.isfinite(got_r[0, 1]) and np.isnan(got_m[0]).all()      # a NaN channel poisons that channel and both moments
    assert got_r[1, 1] == np.inf and np.isnan(got_r[3]).all() and got_r[4, 0] == np.inf
    assert np.isfinite(got_r[5:]).all() and np.isfinite(got_m[5:]).all()                       # ... and no other ray


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_raygen_hot_words(prog, tmp_path, n):
    samples = 3
    rng = np.random.default_rng(n)
    o = (rng.random((n, 3)) * 4 - 2).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)                                         # not normalised: the words are the caller's
    d[0] = [0.0, -0.0, 2.5]
    raw = run(prog, tmp_path, (1, n, samples, 1, 0), [o, d], "g")
    stride = struct.unpack_from("<i", raw)[0]
    P = n * samples
    assert stride == (P + 63) // 64 * 64 and len(raw) == 4 + 4 * R.HOT_FIELDS * stride
    hot = np.frombuffer(raw, np.uint32, R.HOT_FIELDS * stride, 4).reshape(R.HOT_FIELDS, stride)
    want = R.raygen_words(o, d, samples)
    assert sorted(want) == [f for f in range(R.HOT_FIELDS) if not R.HF_HIT < f < R.HF_HIT + 4]      # every field of the block is stated
    for field, w in want.items():
        if field == R.HF_HIT:
            got = hot[R.HF_HIT:R.HF_HIT + 4].reshape(-1)[:4 * P].reshape(P, 4)                      # 16-byte records from the field's base on
        else:
            got = hot[field, :P]
        assert np.array_equal(got, w), (n, field)
    # nothing outside the P slots is written (the program plants a pattern)
    pad = np.ones((R.HOT_FIELDS, stride), bool)
    for field in want:
        if field == R.HF_HIT:
            pad[R.HF_HIT:R.HF_HIT + 4].reshape(-1)[:4 * P] = False
        else:
            pad[field, :P] = False
    assert (hot[pad] == 0xDEADBEEF).all()
