"""The numpy reference of art_aovs_rays_device (tests/aov_rays_ref.py) held to the header's sentences without a GPU: its group mean
for K = 4 is test_gpu_aov.mean4 word for word, K = 1 is the identity, the position rounds once per operation; and the Python wrappers
refuse a bad dtype, shape or group before any library call."""
import numpy as np
import pytest

import aov_rays_ref as ref

F = np.float32
U = np.uint32


def words(a):
    return np.ascontiguousarray(a, F).view(U)


def hard_values(n, seed):
    """[n] float32: ordinary values of mixed sign and magnitude, subnormals (also ones whose quarter is inexact), +-inf, +-0, Float'Last"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(F)
    sub = (rng.integers(1, 1 << 23, n).astype(U) | (rng.integers(0, 2, n).astype(U) << U(31))).view(F)      # every subnormal pattern, both signs
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 3.4028234663852886e38, -3.4028234663852886e38, 1e-45, -1e-45, 3e-45, 1.1754944e-38], F)
    kind = rng.integers(0, 4, n)
    return np.where(kind == 0, sub, np.where(kind == 1, special[rng.integers(0, len(special), n)], v)).astype(F)


def test_group_mean_of_four_is_mean4_word_for_word():
    from test_gpu_aov import mean4
    n = 200000
    v = np.stack([hard_values(n, 11 + s) for s in range(4)])             # [4, n]: the layout mean4 takes
    v[:, :8] = np.array([[1e-45, 1e-45, 1e-45, 0.0], [3e-45, 0.0, 0.0, 0.0], [-1e-45, -1e-45, 0.0, 0.0], [np.inf, -np.inf, 1.0, 1.0],
                         [np.inf, 1.0, 1.0, 1.0], [3e38, 3e38, -3e38, -3e38], [1.0, 1e-8, -1.0, 1e-8], [-0.0, -0.0, -0.0, -0.0]], F).T
    with np.errstate(all="ignore"):
        want = mean4(v)
    got = ref.group_mean(np.ascontiguousarray(v.T), 4)
    same = (words(got) == words(want)) | (np.isnan(got) & np.isnan(want))      # (inf - inf: a NaN either way; its payload is the machine's)
    assert same.all(), np.argwhere(~same)[:5]
    sub = np.abs(want) < F(1.1754944e-38)
    assert (sub & (want != 0)).sum() > 1000 and np.isinf(want).sum() > 1000 and np.isnan(want).sum() > 10      # the hard inputs reached the hard outputs
    ulp = np.array([1, 3], U).view(F)                                        # the smallest subnormal and three of it
    assert ref.group_mean(np.array([[ulp[1], 0.0, 0.0, 0.0]], F), 4)[0] == ulp[0]        # 3 ulp / 4 rounds to 1 ulp, as 3 ulp * 0.25f does
    v3 = np.stack([v, v], -1)                                                # float3-like planes fold per component
    assert np.array_equal(words(ref.group_mean(np.ascontiguousarray(v3.transpose(1, 0, 2)), 4)[:, 0]), words(got))


def test_group_of_one_is_the_identity():
    v = hard_values(100000, 5)
    v[:3] = [np.nan, -0.0, 1e-45]
    got = ref.group_mean(v[:, None], 1)
    assert np.array_equal(words(got), words(v))


def test_other_group_sizes_fold_from_the_left():
    a = np.array([[1.0, 1e-8, 1e-8, -1.0, 3.0]], F)                          # ((((1 + 1e-8) + 1e-8) - 1) + 3) / 5: the small terms are lost
    assert ref.group_mean(a, 5)[0] == F(3.0) / F(5.0)
    b = np.array([[1.0, 2.0, 4.0]], F)
    assert words(ref.group_mean(b, 3))[0] == words(np.array([F(7.0) / F(3.0)]))[0]
    c = np.full((1, 16), 0.1, F)
    acc = F(0.1)
    for _ in range(15):
        acc = F(acc + F(0.1))
    assert ref.group_mean(c, 16)[0] == F(acc / F(16.0))


def test_position_rounds_after_the_multiply_and_after_the_add():
    # t * d = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 (a tie, to even); a fused multiply-add would keep the 2^-24
    t = F(1.0 + 2.0 ** -12); d = F(1.0 + 2.0 ** -12); o = F(-(1.0 + 2.0 ** -11))
    fused = F(float(t) * float(d) + float(o))                                # exact in binary64, rounded once
    assert fused == F(2.0 ** -24)
    got = ref.position(np.array([[o, o, 0.0]], F), np.array([[d, -d, 3.0]], F), np.array([t], F))
    assert got[0, 0] == F(0.0) and got[0, 0] != fused
    assert got[0, 1] == F(-2.0) * F(1.0 + 2.0 ** -11) and got[0, 2] == F(3.0) * t
    rng = np.random.default_rng(3)
    o, d, t = (rng.standard_normal((1000, 3)).astype(F), rng.standard_normal((1000, 3)).astype(F), rng.random(1000).astype(F))
    two_step = (o + (t[:, None] * d).astype(F)).astype(F)
    assert np.array_equal(words(ref.position(o, d, t)), words(two_step))
    once = (o.astype(np.float64) + t[:, None].astype(np.float64) * d.astype(np.float64)).astype(F)
    assert (words(once) != words(two_step)).any()                            # the two roundings are visible on ordinary values too


def test_the_reference_on_hand_made_hit_words():
    """two groups of two rays: hit + miss, miss + miss; every plane from the header's table"""
    raw = np.zeros((4, 11), np.int32); f = raw.view(F)
    raw[0] = [0, 1, 2, 77, 5, 1, 0, 0, 0, 0, 0]; f[0, 0] = 2.0; f[0, 6:9] = [0.0, 1.0, 0.0]
    for i in (1, 2, 3):
        raw[i, 1:6] = [0, -1, -1, -1, -1]; f[i, 0] = 3.4028234663852886e38
    o = np.array([[1.0, 2.0, 3.0]] * 4, F); d = np.array([[0.5, 0.0, -1.0]] * 4, F)
    table = np.array([[0.1, 0.1, 0.1], [0.2, 0.4, 0.8]], F)
    got = ref.aov_rays_ref(raw, o, d, 2, (0.5, 0.25, 1.0), table)
    assert got["albedo"].tolist() == [[F(F(0.2) + F(0.5)) / F(2), F(F(0.4) + F(0.25)) / F(2), F(F(0.8) + F(1.0)) / F(2)], [0.5, 0.25, 1.0]]
    assert got["normal"].tolist() == [[0.0, 0.5, 0.0], [0.0, 0.0, 0.0]] and got["position"].tolist() == [[1.0, 1.0, 0.5], [0.0, 0.0, 0.0]]
    assert got["depth"].tolist() == [1.0, 0.0] and got["alpha"].tolist() == [0.5, 0.0]
    assert got["prim_type"].tolist() == [2, -1] and got["prim_index"].tolist() == [77, -1] and got["mat"].tolist() == [1, -1]
    assert set(got) == set(ref.PLANES)


def test_python_refuses_bad_arguments_before_any_call(art):
    torch = pytest.importorskip("torch")
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU: art_init fails first)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    be.lib = NoCalls()
    o = torch.zeros((8, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="unknown plane 'nope'"):
        be.aovs_rays_torch(o, o, want=("depth", "nope"))
    with pytest.raises(ValueError, match="unknown plane"):
        be.aovs_rays_torch(o, o, out={"motion": o})
    with pytest.raises(art.ArtError, match="at least one plane"):
        be.aovs_rays_torch(o, o, want=())
    with pytest.raises(art.ArtError, match="is not in want"):
        be.aovs_rays_torch(o, o, want=("depth",), out={"alpha": torch.zeros(8)})
    for group in (0, 17, -1, 2.0, "4", True, None):
        with pytest.raises(art.ArtError, match="group must be an integer 1..16"):
            be.aovs_rays_torch(o, o, group=group)
    with pytest.raises(art.ArtError, match="8 rays are not a multiple of group 3"):
        be.aovs_rays_torch(o, o, group=3)
    with pytest.raises(art.ArtError, match="origins: a \\[N, 3\\] float32 tensor"):
        be.aovs_rays_torch([[0, 0, 0]], o)
    with pytest.raises(art.ArtError, match="origins: dtype"):
        be.aovs_rays_torch(o.double(), o)
    with pytest.raises(art.ArtError, match="origins: shape"):
        be.aovs_rays_torch(torch.zeros((8, 4)), o)
    with pytest.raises(art.ArtError, match="dirs: shape"):
        be.aovs_rays_torch(o, torch.zeros((9, 3)))
    with pytest.raises(art.ArtError, match="dirs: dtype"):
        be.aovs_rays_torch(o, o.to(torch.float16))
    with pytest.raises(art.ArtError, match="tnear: shape"):
        be.aovs_rays_torch(o, o, tnear=torch.zeros(7))
    with pytest.raises(art.ArtError, match="tfar: dtype"):
        be.aovs_rays_torch(o, o, tfar=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(art.ArtError, match="background takes 3 floats"):
        be.aovs_rays_torch(o, o, background=(0.0, 0.0))
    with pytest.raises(art.ArtError, match="out\\['depth'\\]: shape"):
        be.aovs_rays_torch(o, o, group=4, out={"depth": torch.zeros(8)})
    with pytest.raises(art.ArtError, match="out\\['mat'\\]: dtype"):
        be.aovs_rays_torch(o, o, out={"mat": torch.zeros(8)})
    with pytest.raises(art.ArtError, match="out\\['normal'\\]: the tensor must be contiguous"):
        be.aovs_rays_torch(o, o, out={"normal": torch.zeros((8, 6))[:, ::2]})
    with pytest.raises(art.ArtError, match="origins: must be a GPU tensor"):
        be.aovs_rays_torch(o, o)
    assert tuple(art.aov_rays.RAY_PLANES) == ref.PLANES
