"""The two pieces of host logic of a render pass (csrc/art_pass_plan.h), compiled by g++ (tests/pass_plan_host) and driven without a GPU:
plan_batch -- the batch shape -- against its Python mirror in test_gpu_batch_shape.py, and ShadeTrial -- the sequence of the shade
stage's items-per-thread trial, which the GPU suite only sees as "whichever value ran, the frame is the same"."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from test_gpu_batch_shape import CAPS, H, W, plan

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "pass_plan_host")])
    L = C.CDLL(os.path.join(HERE, "pass_plan_host", "libpass_plan_host.so"))
    ip = C.POINTER(C.c_int)
    L.pp_plan_batch.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip]
    L.pp_plan_batch.restype = None
    L.pp_trial_new.restype = C.c_void_p
    for name, args in (("free", []), ("reset", []), ("next", [C.c_int64, C.c_int, C.c_int, ip, ip]), ("add", [C.c_int, C.c_uint, C.c_double]),
                       ("decide", []), ("state", [C.POINTER(C.c_int64), C.POINTER(C.c_double)]), ("tag", [C.c_int, C.c_int])):
        f = getattr(L, "pp_trial_" + name)
        f.argtypes = [C.c_void_p] + args
        f.restype = C.c_int if name in ("decide", "tag") else None
    L.pp_tag_encode.argtypes = [C.c_int, C.c_int, C.c_uint]
    L.pp_tag_decode.argtypes = [C.c_int, ip, ip, ip]
    L.pp_tag_decode.restype = None
    return L


def plan_batch(L, npix, S, per, cap):
    pc, sc = C.c_int(), C.c_int()
    L.pp_plan_batch(npix, S, per, cap, C.byref(pc), C.byref(sc))
    return pc.value, sc.value


class Trial:
    """a ShadeTrial of the library"""

    def __init__(self, L):
        self.L, self.h = L, L.pp_trial_new()

    def __del__(self):
        self.L.pp_trial_free(self.h)

    def next(self, paths, pinned=0, record=True):
        trial, per = C.c_int(), C.c_int()
        self.L.pp_trial_next(self.h, paths, pinned, 1 if record else 0, C.byref(trial), C.byref(per))
        return trial.value, per.value

    def reset(self):
        self.L.pp_trial_reset(self.h)

    def add(self, trial, gen, ms):
        self.L.pp_trial_add(self.h, trial, gen, ms)

    def decide(self):
        return bool(self.L.pp_trial_decide(self.h))

    def tag(self, kind, trial=0):
        return self.L.pp_trial_tag(self.h, kind, trial)

    def state(self):
        i, ms = (C.c_int64 * 4)(), (C.c_double * 2)()
        self.L.pp_trial_state(self.h, i, ms)
        return dict(phase=i[0], per=i[1], redo=i[2], gen=i[3], ms=(ms[0], ms[1]))


# ---- the batch plan ---------------------------------------------------------------------------------------------------------------
NPIX = (1, 255, 256, 257, 500, 512, 6144, 2073600)
SAMPLES = (1, 4, 8, 12, 32, 64, 1040)
CAP = (1024, 4000, 5000, 20000, 65536, 128 << 20)


def test_the_plan_is_its_python_mirror_and_fits(lib):
    """pc * sc <= max(cap, per) in every case, without exception: samples first is only taken with cap // S >= min(npix, 256) >= 1, so
    pc = min(npix, cap // S) pixels with S samples fit; pixels first has pc <= cap // per, so cap // pc >= per, and sc is at most cap // pc."""
    n = 0
    for npix, S, cap, per in itertools.product(NPIX, SAMPLES, CAP, (1, 4)):
        if S % per:
            continue
        pc, sc = got = plan_batch(lib, npix, S, per, cap)
        assert got == plan(npix, S, cap, per), (npix, S, cap, per)
        assert 1 <= pc <= npix and per <= sc <= S and sc % per == 0, (npix, S, cap, per, got)
        assert pc * sc <= max(cap, per), (npix, S, cap, per, got)
        n += 1
    assert n == len(NPIX) * len(CAP) * (len(SAMPLES) + len(SAMPLES) - 1)      # S = 1 has no per = 4


def test_the_plan_has_the_pinned_shapes(lib):
    """those of test_gpu_batch_shape.py: test_the_plan_has_the_shapes_this_file_is_about and test_two_passes_of_8_vthreads_equal_one_of_16"""
    assert plan_batch(lib, W * H, 8, 4, CAPS[0]) == (W * H, 8)
    assert plan_batch(lib, W * H, 8, 4, CAPS[1]) == (625, 8)
    assert plan_batch(lib, W * H, 8, 4, CAPS[2]) == (2048, 8)
    assert plan_batch(lib, 32 * 16, 1040, 4, 1024) == (256, 4)
    assert plan_batch(lib, W * H, 8, 4, 1024) == (256, 4)
    assert plan_batch(lib, W * H, 64, 4, 20000) == (312, 64) and plan_batch(lib, W * H, 32, 4, 20000) == (625, 32)
    assert plan_batch(lib, 5, 4, 4, 1) == (1, 4)          # cap = max(cap, per): one group of one pixel


# ---- the trial --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms_a, ms_b, kept", [(5.0, 4.0, 2), (4.0, 5.0, 4), (4.0, 4.0, 4)])
def test_equal_batches(lib, ms_a, ms_b, kept):
    t = Trial(lib)
    g = t.state()["gen"]
    assert [t.next(100) for _ in range(6)] == [(0, 4), (1, 4), (2, 2), (0, 4), (0, 4), (0, 4)]
    assert t.state()["phase"] == 3 and t.state()["gen"] == g
    t.add(1, g, ms_a)
    t.add(2, g, ms_b)
    assert t.state()["ms"] == (ms_a, ms_b)
    assert t.decide() and not t.decide()
    assert t.state()["phase"] == 4 and t.state()["per"] == kept
    assert [t.next(100), t.next(7)] == [(0, kept), (0, kept)]
    assert t.tag(1) == 1                                   # nothing is tagged any more


def test_decide_waits_for_both_trials(lib):
    t = Trial(lib)
    for n in range(3):                                    # before the warm batch, after it, after trial A
        assert not t.decide() and t.state()["phase"] == n
        t.next(100)
    assert t.state()["phase"] == 3


def test_sizes_that_keep_changing(lib):
    t = Trial(lib)
    g = t.state()["gen"]
    gens = []
    for P, want in zip((10, 20, 30, 40, 50, 60), [(0, 4), (1, 4), (1, 4), (1, 4), (1, 4), (0, 4)]):
        assert t.next(P) == want
        gens.append(t.state()["gen"])
    assert gens == [g, g, g + 1, g + 2, g + 3, g + 3]     # one bump for each re-done trial A
    s = t.state()
    assert s["phase"] == 4 and s["per"] == 4 and s["redo"] == 4
    assert not t.decide()
    assert [t.next(60), t.next(60), t.next(10)] == [(0, 4)] * 3 and t.state()["gen"] == g + 3


def test_a_redone_trial_that_then_meets_its_size(lib):
    t = Trial(lib)
    g = t.state()["gen"]
    assert [t.next(P) for P in (10, 20, 30, 30, 30)] == [(0, 4), (1, 4), (1, 4), (2, 2), (0, 4)]
    s = t.state()
    assert s["phase"] == 3 and s["redo"] == 1 and s["gen"] == g + 1
    t.add(1, g + 1, 3.0)
    t.add(2, g + 1, 2.0)
    assert t.decide() and t.next(30) == (0, 2)


def test_add_drops_an_older_generation_and_counts_its_alias(lib):
    """a pair's tag keeps two bits of the generation: four generations on, an old trial's pairs count again (known; pinned here, not hidden)"""
    t = Trial(lib)
    g = t.state()["gen"]
    assert [t.next(P) for P in (10, 20, 30)] == [(0, 4), (1, 4), (1, 4)]      # trial A of generation g, then again as g + 1
    for old in (g, g + 2, g + 3):
        t.add(1, old, 100.0)
    assert t.state()["ms"] == (0.0, 0.0)
    t.add(1, g + 1, 5.0)
    t.add(1, g + 1 + 4, 0.5)
    t.add(1, (g + 1) & 3, 0.25)                           # (what a decoded tag carries)
    assert t.state()["ms"] == (5.75, 0.0)
    t.add(0, g + 1, 9.0)                                  # not a trial's pair
    t.add(3, g + 1, 9.0)
    t.add(2, g + 1, 1.0)
    assert t.state()["ms"] == (5.75, 1.0)


def test_a_new_trial_zeroes_its_sum(lib):
    t = Trial(lib)
    g = t.state()["gen"]
    t.next(10), t.next(20)
    t.add(1, g, 5.0)
    assert t.next(30) == (1, 4) and t.state()["ms"] == (0.0, 0.0)


def test_reset_returns_to_the_warm_batch(lib):
    t = Trial(lib)
    g = t.state()["gen"]
    for P in (10, 20, 30, 40, 50, 60):
        t.next(P)
    assert t.state()["phase"] == 4
    t.reset()
    s = t.state()
    assert s["phase"] == 0 and s["redo"] == 0 and s["gen"] == g + 4
    assert [t.next(100) for _ in range(4)] == [(0, 4), (1, 4), (2, 2), (0, 4)]
    t.reset()                                             # with both trials enqueued: their pairs no longer count
    assert t.state()["phase"] == 0 and t.state()["gen"] == g + 5
    t.add(1, g + 4, 5.0)
    assert t.state()["ms"][0] == 0.0 and not t.decide()


@pytest.mark.parametrize("pinned, record, per", [(2, True, 2), (4, True, 4), (2, False, 2), (4, False, 4), (0, False, 4)])
def test_a_pinned_option_or_the_plain_schedule_never_starts_a_trial(lib, pinned, record, per):
    t = Trial(lib)
    before = t.state()
    assert [t.next(P, pinned, record) for P in (100, 100, 100, 50, 100)] == [(0, per)] * 5
    assert t.state() == before and before["phase"] == 0
    # ... nor moves one that is under way
    assert [t.next(100), t.next(100)] == [(0, 4), (1, 4)]
    mid = t.state()
    assert t.next(100, pinned, record) == (0, per) and t.state() == mid and mid["phase"] == 2
    assert t.next(100) == (2, 2)


def test_tag_round_trip(lib):
    for kind, trial, gen in itertools.product(range(4), range(3), range(8)):
        tag = lib.pp_tag_encode(kind, trial, gen)
        assert 0 <= tag < 256 and tag == kind | trial << 4 | ((gen & 3) << 6 if trial else 0)
        k, t, g = C.c_int(), C.c_int(), C.c_int()
        lib.pp_tag_decode(tag, C.byref(k), C.byref(t), C.byref(g))
        assert (k.value, t.value, g.value) == (kind, trial, gen & 3 if trial else 0)


def test_a_trials_tag_carries_its_generation(lib):
    t = Trial(lib)
    t.next(10), t.next(20), t.next(30), t.next(40)        # generation + 2
    gen = t.state()["gen"]
    assert gen & 3 == 2
    assert t.tag(1, 1) == lib.pp_tag_encode(1, 1, gen) == 1 | 1 << 4 | 2 << 6
    assert t.tag(1) == 1 and t.tag(0) == 0 and t.tag(3) == 3
