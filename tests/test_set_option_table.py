"""art_set_option's table, pinned: for every option name the return code and the art_last_error() text at its bounds, inside them and
just outside them, plus an unknown name and a null one, as recorded from the library before the option fields moved into one struct
(tests/golden/set_option_table.json).  art_set_option touches no device, so this runs without a GPU.  The replay runs in a child
process of its own: the library is a process-wide singleton, and the values set here must not reach another test.

    python tests/test_set_option_table.py --record      records the fixture again from the built library (after a deliberate change)
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "set_option_table.json")

# name -> the values tried, in this order: below the range, its lower bound, inside, its upper bound, above it (switches and free
# integers: a few values)
VALUES = {
    "trace_kernel": [-1, 0, 1, 2],
    "queue_segments": [0, 1, 2, 3, 4, 8, 9, 16],
    "batch_paths": [1023, 1024, 1 << 20, 1 << 27, (1 << 27) + 1],
    "paths_spread": [-2, -1, 0, 64, 65536, 65537],
    "spread_fail_at": [-1, 0, 5],
    "inject_lost": [0, 1],
    "blocks_per_cu": [-1, 0, 2],
    "query_slice": [0, 1, 1000, 1 << 28, (1 << 28) + 1],
    "count_tests": [0, 1, 2],
    "camera_dedup": [-1, 0, 1, 2],
    "shadow_anyhit": [0, 1, 2],
    "skip_null_shadow": [0, 1, 2],
    "inst_coop": [0, 1, 2],
    "shade_per": [-1, 0, 1, 2, 3, 4, 5],
    "ray_chunk": [0, 15, 16, 17, 48, 4096, 4097, 4112],
    "refill_min": [0, 1, 2, 8, 9],
    "node_min": [-1, 0, 4, 8, 9],
    "bvh_width": [3, 4, 5, 7, 8, 9],
    "lds_stack_cap": [-1, 0, 14, 160, 161],
    "bvh_max_leaf": [-1, 0, 4, 8, 9],
    "inst_open": [-1, 0, 16, 4096, 4097],
    "bvh_spatial_splits": [0, 1, 2],
    "bvh_builder": [-1, 0, 2, 3, 4],
    "bvh_ploc_radius": [0, 1, 16, 64, 65],
    "bvh_leaf_base_milli": [-1, 0, 1500],
    "bvh_tri_cost_milli": [-1, 0, 1500],
    "bvh_node_cost_milli": [-1, 0, 1500],
    "no_such_option": [0],
    None: [0],
}

CHILD = """
import json, sys
sys.path.insert(0, %r)
import __graft_entry__ as g
L = g.load_package().load_library()          # dlopen + symbol binding; no GPU call
out = []
for name, value in json.load(sys.stdin):
    rc = L.art_set_option(None if name is None else name.encode(), value)
    out.append({"name": name, "value": value, "rc": rc, "error": L.art_last_error().decode()})
json.dump(out, sys.stdout)
"""


def _replay(calls):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], input=json.dumps(calls), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_set_option_table_is_unchanged():
    want = json.load(open(FIXTURE))
    assert {e["name"] for e in want} == set(VALUES)                 # the fixture covers every name of the table above
    got = _replay([[e["name"], e["value"]] for e in want])
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, "art_set_option(%r, %d): got rc %d %r, recorded rc %d %r" % (w["name"], w["value"], g["rc"], g["error"], w["rc"], w["error"])
    assert any(e["rc"] != 0 for e in want) and any(e["rc"] == 0 for e in want)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    table = _replay([[name, v] for name, values in VALUES.items() for v in values])
    with open(FIXTURE, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    print("recorded %d calls, %d refused" % (len(table), sum(e["rc"] != 0 for e in table)))
