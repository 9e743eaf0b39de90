"""art_set_camera on the GPU: after the call the accum of a pass and all seven feature planes are a fresh art_upload_scene's with that
camera, bit for bit -- translated, rotated, and outside the uploaded scene's reach (on an instanced scene that re-pads the meshes' boxes),
then back inside; a pass enqueued before the call keeps the old camera; the same under art_init_devices with two contexts on one GPU
(a child process: the library is a process-wide singleton); the refusals."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
W = H = 48


def yaw(a):
    m = np.eye(4, dtype=F)
    m[0, 0] = m[2, 2] = np.cos(a); m[0, 2] = np.sin(a); m[2, 0] = -np.sin(a)
    return m


BASE = ((0.0, 2.55, 12.5), np.eye(4, dtype=F))
CAMERAS = [("translated", ((0.7, 2.2, 11.0), np.eye(4, dtype=F))), ("rotated", ((0.0, 2.55, 12.5), yaw(0.3))),
           ("outside_reach", ((40.0, 2.55, 60.0), yaw(0.55))), ("back_inside", ((-0.4, 2.9, 12.0), yaw(-0.1)))]


def make_scene(kind, cam):
    from ada_ray_tracer_amd import scenes
    sd = scenes.synthetic_scene(2000, 3) if kind == "flat" else scenes.instanced_scene(6, 200)
    for k in range(3):
        sd.desc.cam_pos[k] = cam[0][k]
    for k in range(16):
        sd.desc.cam_matrix[k] = float(cam[1].reshape(-1)[k])
    return sd


def snapshot(art, be):
    """one PT_MIS pass from a fresh viewport (the accum) and the seven feature planes, as bits"""
    p = art.Backend.pass_params(art.PT_MIS, True, 6, 1, seed=9)
    be.resize(W, H)
    accum, _, spp = be.render_pass(p, 0)
    aovs = be.render_aovs_torch(p)
    torch.cuda.synchronize()
    out = {"accum": accum.view(np.uint32).copy()}
    for name, t in aovs.items():
        a = t.cpu().numpy()
        out[name] = a.view(np.uint32).copy() if a.dtype == np.float32 else a.copy()
    assert spp == 4 and len(out) == 8
    return out


def equal(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_set_camera_equals_a_fresh_upload(art, backend, kind):
    want = {}
    for name, cam in [("base", BASE)] + CAMERAS:
        backend.upload_scene(make_scene(kind, cam))
        want[name] = snapshot(art, backend)
    assert equal(want["base"], want["translated"]) and equal(want["base"], want["rotated"]) and want["outside_reach"]["accum"].any()
    backend.upload_scene(make_scene(kind, BASE))
    for name, cam in CAMERAS:
        backend.set_camera(*cam)
        assert equal(snapshot(art, backend), want[name]) == [], name
    if kind == "instanced":                      # the camera outside the reach raised the extent the pads follow
        info, rc = art.two_level_arrays(backend.lib.art_export_two_level)
        assert rc == 0 and float(info["scene_extent"]) == 60.0 and info["updated"] == 1


def test_a_pass_enqueued_before_the_call_keeps_the_old_camera(art, backend):
    p = art.Backend.pass_params(art.PT_MIS, True, 6, 1, seed=9)
    cam = CAMERAS[0][1]
    backend.upload_scene(make_scene("flat", cam))
    new = snapshot(art, backend)["accum"]
    backend.upload_scene(make_scene("flat", BASE))
    old = snapshot(art, backend)["accum"]
    backend.resize(W, H)
    spp = backend.render_pass_device(p, 0)                 # enqueued; nothing synchronises before the camera changes
    backend.set_camera(*cam)
    got, _ = backend.download(spp, want_screen=False)
    assert np.array_equal(got.view(np.uint32), old) and not np.array_equal(old, new)
    backend.resize(W, H)
    got, _, _ = backend.render_pass(p, 0)
    assert np.array_equal(got.view(np.uint32), new)


def test_refusals(art, backend):
    L = backend.lib
    pos, m = (C.c_float * 3)(0, 2.55, 12.5), (C.c_float * 16)(*[float(v) for v in np.eye(4).reshape(-1)])
    backend.upload_scene(make_scene("flat", BASE))
    before = snapshot(art, backend)

    def refused(a, b, text):
        assert L.art_set_camera(a, b) != 0 and text in L.art_last_error().decode(), (text, L.art_last_error().decode())
    refused(None, C.byref(m), "null cam_pos or cam_matrix")
    refused(C.byref(pos), None, "null cam_pos or cam_matrix")
    for bad in (float("nan"), float("inf")):
        refused(C.byref((C.c_float * 3)(0, bad, 0)), C.byref(m), "not finite")
        mm = (C.c_float * 16)(*list(m)); mm[6] = bad
        refused(C.byref(pos), C.byref(mm), "not finite")
    assert equal(snapshot(art, backend), before) == []          # nothing changed
    L.gcore_init_and_clear()
    v = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0); idx = (C.c_int * 3)(0, 1, 2)
    L.gcore_instance_meshes(L.gcore_add_mesh_3f(v, 3, idx, 3), (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1), 1)
    L.gcore_commit_scene()
    refused(C.byref(pos), C.byref(m), "gcore_commit_scene")
    L.gcore_destroy()


SCRIPT = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
art = ge.load_package()
import test_gpu_set_camera as T
out = {}
be = art.Backend(devices=[0, 0])
try:
    out["no_scene"] = False
    be.set_camera(*T.BASE)
except art.ArtError as e:
    out["no_scene"] = "no scene uploaded" in str(e)
for kind in ("flat", "instanced"):
    want = {}
    for name, cam in T.CAMERAS:
        be.upload_scene(T.make_scene(kind, cam))
        want[name] = T.snapshot(art, be)
    be.upload_scene(T.make_scene(kind, T.BASE))
    base = T.snapshot(art, be)
    for name, cam in T.CAMERAS:
        be.set_camera(*cam)
        out[kind + "_" + name] = T.equal(T.snapshot(art, be), want[name])
    out[kind + "_moved"] = bool(T.equal(base, want["translated"]))
    p = art.Backend.pass_params(art.PT_MIS, True, 6, 1, seed=9)
    be.set_camera(*T.BASE)
    be.resize(T.W, T.H)
    spp = be.render_pass_device(p, 0)
    be.set_camera(*T.CAMERAS[0][1])
    got, _ = be.download(spp, want_screen=False)
    out[kind + "_old_camera_kept"] = bool(np.array_equal(got.view(np.uint32), base["accum"]))
be.shutdown()
print("RESULT " + json.dumps(out))
'''


def test_two_contexts_on_one_gpu(art):
    r = subprocess.run([sys.executable, "-c", SCRIPT, art.ROOT], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(line[0][7:])
    want = {"no_scene": True}
    for kind in ("flat", "instanced"):
        want.update({kind + "_" + name: [] for name, _ in CAMERAS})
        want.update({kind + "_moved": True, kind + "_old_camera_kept": True})
    assert out == want
