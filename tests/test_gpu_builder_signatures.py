"""The trees the three GPU builders leave (csrc/art_lbvh.hip: 1 = LBVH, 2 = PLOC; csrc/art_sah.hip: 3 = binned SAH) are pinned: the
numbering-independent signature of tests/tree_sig.py, the node count and the stack bound of the tree art_export_bvh returns, for both
node widths and for meshes of 2 triangles (a root with leaf children only), 5 (the first tree with an inner child), 300 (several collapse
levels) and 2049 (one more than the SAH builder's chunk: the big-node path and the small-node path both feed the collapse).  Builders 1
and 2 number their nodes by atomics, so the signature is pinned, not the bytes.  tests/golden/gpu_builder_signatures.json holds the
record;

    python tests/test_gpu_builder_signatures.py --record

writes it from the package as it stands, on a machine with a GPU.  It was recorded once, from the builders as they were before the packet
writer and the build's scaffold moved into csrc/art_gpu_build.h, and it is not edited by hand: a change that alters a builder's trees on
purpose records again and says so."""
import json
import os
import subprocess
import sys

import pytest

from tree_sig import tree_signature

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gpu_builder_signatures.json")
BUILDERS = (1, 2, 3)
WIDTHS = (4, 8)
SIZES = (2, 5, 300, 2049)


def signature(art, backend, builder, width, ntris):
    """(signature, n_nodes, max_stack) of the tree `builder` leaves for the suite's soup of `ntris` triangles (0: the host builder)"""
    from ada_ray_tracer_amd import scenes
    try:
        backend.set_option("bvh_width", width)
        backend.set_option("bvh_builder", builder)
        backend.upload_scene(scenes.synthetic_scene(ntris, 3))
        nodes, tris, info = backend.export_bvh()
    finally:
        backend.set_option("bvh_builder", art.DEFAULT_BVH_BUILDER)
        backend.set_option("bvh_width", 4)
    assert info.n_tris == ntris and info.node_width == width
    return {"signature": list(tree_signature(nodes, tris, info)), "n_nodes": int(info.n_nodes), "max_stack": int(info.max_stack)}


def key(builder, width, ntris):
    return "builder%d-w%d-%d" % (builder, width, ntris)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("ntris", SIZES)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_the_builder_leaves_the_recorded_tree(art, backend, golden, builder, width, ntris):
    want = golden["trees"][key(builder, width, ntris)]
    got = signature(art, backend, builder, width, ntris)
    assert got == want
    if builder == 3:                       # the SAH builder restates the host builder: the unchanged host builder is a second witness
        assert signature(art, backend, 0, width, ntris) == got


def test_the_record_holds_every_case(golden):
    assert sorted(golden["trees"]) == sorted(key(b, w, n) for b in BUILDERS for w in WIDTHS for n in SIZES)
    assert len(golden["trees"]) == 24 and golden["recorded_from"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_builder_signatures.py --record")
    sys.path.insert(0, os.path.dirname(HERE))
    import __graft_entry__ as ge
    art = ge.load_package()
    art.load_library()
    be = art.Backend(0)
    commit = os.environ.get("RECORD_COMMIT") or subprocess.check_output(["git", "-C", HERE, "rev-parse", "--short", "HEAD"], text=True).strip()
    rec = {"recorded_from": commit, "trees": {key(b, w, n): signature(art, be, b, w, n) for b in BUILDERS for w in WIDTHS for n in SIZES}}
    be.shutdown()
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("recorded %s" % GOLDEN)
