"""Per-function known-answer tests of the DEVICE build: the product's ART_HD functions (csrc/art_math.h, art_isect.h, art_shade.h) compiled by
hipcc for gfx950 with the product's flags (tests/device_kat, one item per lane) against
  * the same per-item text compiled by g++ (tests/host_sim hs_kat_run) on the WHOLE input set, word for word -- one relaxation: where both
    are NaN, payload and sign may differ (the x86 default NaN is 0xffc00000, the GPU's 0x7fc00000);
  * the independent Ada transcription (tests/ada_transcription.py) on the edge lists and the first 1000 random items, under the same rule.
The inputs (tests/kat_inputs.py) sit where this arithmetic can go wrong: special-case exponents of apow one ulp either side, the k-rounding
boundaries of sincos, denormal operands of sqrt and division, glass at the critical angle, det at the 1e-25 clamp of the triangle test.
The last four ops are the two ends of a picture: camera_dir per pixel and sample (frames from 1x1 to 4096x2160, rotated and moved cameras,
narrow and wide fields of view) and resolve_pixel / ada_round_u32 / colour_lum (NaN, infinities, negative sums, and for every byte the
input at which it rises and its neighbours one ulp either side); camera_dir and the resolve are also held to float64 references
(tests/test_device_kat_host.py assert_float64).
A device / host difference means a build flag (-ffp-contract=off, correctly rounded divide / sqrt, denormals kept) is no longer honoured
for that function, or an optimisation changed the operation order.  tests/test_device_kat_host.py is the CPU leg (transcription, mpmath)."""
import numpy as np
import pytest

import devkat
import kat_inputs as ki
import kat_refs
import test_device_kat_host as host_leg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", list(devkat.OPS))
def test_device_build_equals_host_build_and_transcription(art, op):
    host = kat_refs.host_runner(art, op)
    dev_out = {}

    def dev(case):
        if id(case) not in dev_out:
            dev_out[id(case)] = devkat.run_device(op, case.words, case.params)
        return dev_out[id(case)]

    n_items = 0
    for case in ki.cases(op):
        got, want = dev(case), host(case)
        bad = kat_refs.differing(op, got, want)
        print("%s/%s: %d items (%d edges), %d differ from the host build" % (op, case.label, got.shape[0], case.n_edge, bad.size))
        assert bad.size == 0, "%s/%s: device and host builds differ on %d of %d items, first: item %d in %s device %s host %s" % (
            op, case.label, bad.size, got.shape[0], bad[0], case.inp[bad[0]].tolist(), got[bad[0]].view(np.float32).tolist(), want[bad[0]].view(np.float32).tolist())
        n_items += got.shape[0]
    assert n_items > 0
    kat_refs.assert_matches_transcription(op, dev)
    kat_refs.assert_coverage(op, kat_refs.run_all(op, dev))
    host_leg.assert_float64(op, dev)               # camera_dir, resolve: the float64 references, within twice the transcription's own deviation
