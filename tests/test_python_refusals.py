"""What the torch-facing wrappers of Backend refuse, and in which words, without a GPU: every case of the table below is a Backend
method and arguments built from CPU tensors; the library behind the Backend is a stub whose art_trace_rays_device returns 0 (the
zero-ray "is there a device?" probe passes) and whose every other entry fails the test.  tests/golden/python_refusals.json holds
the exception class and the message of every case, the signature of every public Backend method and of SceneDesc.__init__, and the
module's public names; the test asserts all of them, the messages byte for byte.

    python tests/test_python_refusals.py --record

writes the JSON from the package as it stands.  It is recorded once, from the binding as it was before its checks were folded into
one plane checker and one device checker, and it is not edited by hand: a wrapper that changes a refusal on purpose records again
and shows the difference in review.

The table reaches every `raise` of Backend that CPU tensors and that stub can reach, and it holds the order cases: a wrong dtype, a
wrong shape, an empty or a strided tensor on the CPU (kind of argument against place), two bad planes at once, and a bad later
plane next to a first plane on the wrong device.  The raise sites it cannot reach, each because a tensor on the CPU is refused for
its place before that line runs (or, for the last two, because the line needs a CUDA stream):

  - bind_accum and bind_moments: "dtype must be", "the tensor must be contiguous", "the tensor is empty" (the device comes first)
  - render_aovs_torch_motion: "cur_pos and prev_pos must both be given or both be None", "cur_pos and prev_pos differ in length"
  - denoise_svgf_torch: "n_colours must be at least 2"
  - temporal_torch: "n_colours must be at least 1"
  - _frame_tensor (compact_mask_torch, render_pass_masked, adaptive_estimate_torch): "dtype must be", "the tensor must be
    contiguous", "the tensor holds %d elements, the frame needs %d" (the device comes first)
  - adaptive_estimate_torch: "want: unknown plane", "want: at least one plane"
  - refit_torch and refit_mesh_torch: the ValueError of the finite-vertex check
  - move_instances_torch: the ValueError of the finite-matrix check
  - the `torch is None` half of the "a torch tensor is required" conditions is the same line as the half the table reaches

What a wrapper does once nothing is refused (allocation, stream, the C calls) is the GPU suite's to pin.
"""
import collections
import inspect
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "python_refusals.json")


class StubLibrary:
    """art_trace_rays_device(...) -> 0; anything else: the wrapper went past its refusals"""

    def __getattr__(self, name):
        if name == "art_trace_rays_device":
            return lambda *args: 0
        raise AssertionError("the library was called")


def stub_backend(art, attrs):
    be = art.Backend.__new__(art.Backend)                 # (Backend() itself needs a GPU)
    be.lib = StubLibrary()
    be.width = be.height = 4
    be._accum_tensor = be._moments_tensor = None
    for name, value in attrs.items():
        setattr(be, name, value)
    return be


def cases(art, torch):
    """[(id, method, args, kwargs, attributes set on the Backend by hand)]"""
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8

    def z(*shape, **kw):
        return torch.zeros(shape, **kw)
    table = []

    def case(ident, method, *args, **kwargs):
        table.append((ident, method, args, kwargs, {}))
    P = art.Backend.pass_params()
    strided = z(4, 3, 4).transpose(1, 2)                  # [4, 4, 3], not contiguous
    cam = ((0.0, 0.0, 0.0), [0.0] * 16)

    # resize: the guards of the tensors bind_accum / bind_moments hold
    table.append(("resize/accum too small", "resize", (4, 4), {}, {"_accum_tensor": z(47)}))
    table.append(("resize/moments too small", "resize", (4, 4), {}, {"_accum_tensor": z(48), "_moments_tensor": z(31)}))

    for bind in ("bind_accum", "bind_moments"):
        case(bind + "/a string", bind, "0x1000")
        case(bind + "/a float", bind, 1.5)
        case(bind + "/on the CPU", bind, z(4, 4, 3))
        case(bind + "/order: float64 on the CPU", bind, z(4, 4, 3, dtype=f64))
        case(bind + "/order: strided on the CPU", bind, strided)
        case(bind + "/order: empty on the CPU", bind, z(0))

    for query in ("trace_rays_torch", "occluded_torch"):
        case(query + "/origins a list", query, [[0.0, 0.0, 0.0]], z(1, 3))
        case(query + "/origins 1-D", query, z(3), z(1, 3))
        case(query + "/origins float64", query, z(4, 3, dtype=f64), z(4, 3))
        case(query + "/origins [4, 2]", query, z(4, 2), z(4, 3))
        case(query + "/dirs a list", query, z(4, 3), [[0.0, 0.0, 1.0]] * 4)
        case(query + "/dirs float64", query, z(4, 3), z(4, 3, dtype=f64))
        case(query + "/dirs [5, 3]", query, z(4, 3), z(5, 3))
        case(query + "/tnear a float", query, z(4, 3), z(4, 3), tnear=0.0)
        case(query + "/tnear [5]", query, z(4, 3), z(4, 3), tnear=z(5))
        case(query + "/tfar float64", query, z(4, 3), z(4, 3), tfar=z(4, dtype=f64))
        case(query + "/tfar [4, 1]", query, z(4, 3), z(4, 3), z(4), z(4, 1))
        case(query + "/on the CPU", query, z(4, 3), z(4, 3), z(4), z(4))
        case(query + "/strided on the CPU", query, z(3, 4).t(), z(4, 3))
        case(query + "/no rays on the CPU", query, z(0, 3), z(0, 3))
        case(query + "/order: origins float64, dirs [5, 3]", query, z(4, 3, dtype=f64), z(5, 3))
        case(query + "/order: origins on the CPU, tfar a list", query, z(4, 3), z(4, 3), tfar=[1.0] * 4)

    case("render_aovs_torch/unknown plane", "render_aovs_torch", P, want=("albedo", "nope"))
    call = "render_aovs_torch_motion"
    case(call + "/unknown plane", call, P, want=("nope",))
    case(call + "/unknown plane before a bad tensor", call, P, want=("nope",), cur_pos=[1.0])
    case(call + "/cur_pos a list", call, P, cur_pos=[[0.0, 0.0, 0.0]], prev_pos=z(1, 3))
    case(call + "/cur_pos float64", call, P, cur_pos=z(5, 3, dtype=f64), prev_pos=z(5, 3))
    case(call + "/prev_pos int32", call, P, prev_pos=z(5, 3, dtype=i32))
    case(call + "/cur_pos 1-D", call, P, cur_pos=z(6), prev_pos=z(6))
    case(call + "/cur_pos [5, 2]", call, P, cur_pos=z(5, 2), prev_pos=z(5, 2))
    case(call + "/cur_pos empty", call, P, cur_pos=z(0, 3), prev_pos=z(0, 3))
    case(call + "/prev_matrices [2, 11]", call, P, prev_matrices=z(2, 11))
    case(call + "/prev_matrices [2, 4, 3] on the CPU", call, P, prev_matrices=z(2, 4, 3))
    case(call + "/prev_matrices [2, 3, 4] on the CPU", call, P, prev_matrices=z(2, 3, 4))
    case(call + "/cur_pos strided", call, P, cur_pos=z(3, 5).t(), prev_pos=z(5, 3))
    case(call + "/on the CPU", call, P, cur_pos=z(5, 3), prev_pos=z(5, 3))
    case(call + "/cur_pos alone on the CPU", call, P, cur_pos=z(5, 3))
    case(call + "/prev_pos alone on the CPU", call, P, want=(), prev_pos=z(5, 3))
    case(call + "/lengths differ on the CPU", call, P, cur_pos=z(5, 3), prev_pos=z(6, 3))
    case(call + "/order: cur_pos float64, prev_pos a list", call, P, cur_pos=z(5, 3, dtype=f64), prev_pos=[1.0])
    case(call + "/order: cur_pos on the CPU, prev_pos float64", call, P, cur_pos=z(5, 3), prev_pos=z(5, 3, dtype=f64))
    case(call + "/order: cur_pos float64 and [5, 2]", call, P, cur_pos=z(5, 2, dtype=f64), prev_pos=z(5, 3))
    case(call + "/order: cur_pos strided and [5, 2]", call, P, cur_pos=z(2, 5).t(), prev_pos=z(5, 3))

    call = "denoise_torch"
    case(call + "/unknown keyword", call, z(4, 4, 3), foo=1)
    case(call + "/unknown keyword before a bad colour", call, None, foo=1)
    case(call + "/color a list", call, [1.0])
    case(call + "/color None", call, None)
    case(call + "/color [4, 4]", call, z(4, 4))
    case(call + "/color [4, 4, 4]", call, z(4, 4, 4))
    case(call + "/color empty", call, z(0, 4, 3))
    case(call + "/color float64", call, z(4, 4, 3, dtype=f64))
    case(call + "/color strided", call, strided)
    case(call + "/on the CPU", call, z(4, 4, 3), z(4, 4, 3), z(4, 4, 3), z(4, 4), out=z(4, 4, 3))
    case(call + "/a plane of the AOV dict is ignored", call, z(4, 4, 3), alpha=[1.0], prim_index=z(2))
    case(call + "/order: color float64 and [4, 4]", call, z(4, 4, dtype=f64))
    case(call + "/order: color float64 and strided", call, strided.to(f64))
    case(call + "/order: color float64, albedo a list", call, z(4, 4, 3, dtype=f64), [1.0])
    case(call + "/order: color on the CPU, albedo a list", call, z(4, 4, 3), [1.0])
    case(call + "/order: color on the CPU, albedo float64", call, z(4, 4, 3), z(4, 4, 3, dtype=f64))
    case(call + "/order: color on the CPU, depth [4, 4, 3]", call, z(4, 4, 3), depth=z(4, 4, 3))
    case(call + "/order: color on the CPU, out strided", call, z(4, 4, 3), out=strided)

    call = "denoise_svgf_torch"
    good = dict(moments=z(4, 4, 2), n_colours=4)
    case(call + "/unknown keyword", call, z(4, 4, 3), foo=1, **good)
    case(call + "/color a list", call, [1.0], **good)
    case(call + "/color [4, 4]", call, z(4, 4), **good)
    case(call + "/color empty", call, z(4, 0, 3), **good)
    case(call + "/moments and variance", call, z(4, 4, 3), variance=z(4, 4), moments=z(4, 4, 2))
    case(call + "/n_colours and variance", call, z(4, 4, 3), variance=z(4, 4), n_colours=4)
    case(call + "/moments and variance before a bad dtype", call, z(4, 4, 3, dtype=f64), variance=z(4, 4), n_colours=4)
    case(call + "/color [4, 4] before moments and variance", call, z(4, 4), variance=z(4, 4), n_colours=4)
    case(call + "/no moments", call, z(4, 4, 3), n_colours=4)
    case(call + "/moments a list", call, z(4, 4, 3), [0.0] * 32, 4)
    case(call + "/moments float64", call, z(4, 4, 3), z(4, 4, 2, dtype=f64), 4)
    case(call + "/moments too small", call, z(4, 4, 3), z(31), 4)
    case(call + "/moments flat and larger on the CPU", call, z(4, 4, 3), z(40), 4)
    case(call + "/moments strided", call, z(4, 4, 3), z(2, 4, 4).permute(1, 2, 0), 4)
    case(call + "/color float64", call, z(4, 4, 3, dtype=f64), **good)
    case(call + "/color strided", call, strided, **good)
    case(call + "/albedo [4, 4]", call, z(4, 4, 3), albedo=z(4, 4), **good)
    case(call + "/normal a list", call, z(4, 4, 3), normal=[1.0], **good)
    case(call + "/depth [4, 4, 3]", call, z(4, 4, 3), depth=z(4, 4, 3), **good)
    case(call + "/out float64", call, z(4, 4, 3), out=z(4, 4, 3, dtype=f64), **good)
    case(call + "/out strided", call, z(4, 4, 3), out=strided, **good)
    case(call + "/variance_out [4, 4, 1]", call, z(4, 4, 3), variance_out=z(4, 4, 1), **good)
    case(call + "/variance [4, 4, 2]", call, z(4, 4, 3), variance=z(4, 4, 2))
    case(call + "/variance float64", call, z(4, 4, 3), variance=z(4, 4, dtype=f64))
    case(call + "/on the CPU", call, z(4, 4, 3), albedo=z(4, 4, 3), normal=z(4, 4, 3), depth=z(4, 4), out=z(4, 4, 3), variance_out=z(4, 4), **good)
    case(call + "/variance on the CPU", call, z(4, 4, 3), variance=z(4, 4))
    case(call + "/n_colours 0 on the CPU", call, z(4, 4, 3), moments=z(4, 4, 2))
    case(call + "/n_colours 1 on the CPU", call, z(4, 4, 3), moments=z(4, 4, 2), n_colours=1)
    case(call + "/a plane of the AOV dict is ignored", call, z(4, 4, 3), mat=[1.0], **good)
    case(call + "/order: moments float64, albedo a list", call, z(4, 4, 3), z(4, 4, 2, dtype=f64), 4, albedo=[1.0])
    case(call + "/order: moments float64 and too small", call, z(4, 4, 3), z(31, dtype=f64), 4)
    case(call + "/order: moments too small and strided", call, z(4, 4, 3), z(31, 2)[:, 0], 4)
    case(call + "/order: color float64, no moments", call, z(4, 4, 3, dtype=f64), n_colours=4)
    case(call + "/order: color on the CPU, albedo float64", call, z(4, 4, 3), albedo=z(4, 4, 3, dtype=f64), **good)
    case(call + "/order: color on the CPU, variance_out a list", call, z(4, 4, 3), variance_out=[1.0], **good)
    case(call + "/order: color on the CPU, depth [4, 4, 3]", call, z(4, 4, 3), depth=z(4, 4, 3), **good)

    call = "temporal_torch"

    def cur(**planes):
        d = dict(color=z(4, 4, 3), moments=z(4, 4, 2))
        d.update(planes)
        return d
    hist = z(3, 2, 6, 4)                                   # (a history's frame size is its own)
    case(call + "/cur a list", call, [z(4, 4, 3)], None, cam, None, 4)
    case(call + "/no color", call, {}, None, cam, None, 4)
    case(call + "/color a list", call, cur(color=[1.0]), None, cam, None, 4)
    case(call + "/color [4, 4]", call, cur(color=z(4, 4)), None, cam, None, 4)
    case(call + "/color empty", call, cur(color=z(0, 4, 3)), None, cam, None, 4)
    case(call + "/color float64", call, cur(color=z(4, 4, 3, dtype=f64)), None, cam, None, 4)
    case(call + "/color strided", call, cur(color=strided), None, cam, None, 4)
    case(call + "/no moments", call, dict(color=z(4, 4, 3)), None, cam, None, 4)
    case(call + "/moments a list", call, cur(moments=[1.0]), None, cam, None, 4)
    case(call + "/moments float64", call, cur(moments=z(4, 4, 2, dtype=f64)), None, cam, None, 4)
    case(call + "/moments too small", call, cur(moments=z(31)), None, cam, None, 4)
    case(call + "/normal [4, 4]", call, cur(normal=z(4, 4)), None, cam, None, 4)
    case(call + "/normal strided", call, cur(normal=strided), None, cam, None, 4)
    case(call + "/depth a list", call, cur(depth=[1.0]), None, cam, None, 4)
    case(call + "/depth [4, 4, 1]", call, cur(depth=z(4, 4, 1)), None, cam, None, 4)
    case(call + "/prim_index float32", call, cur(prim_index=z(4, 4)), None, cam, None, 4)
    case(call + "/prim_index [4]", call, cur(prim_index=z(4, dtype=i32)), None, cam, None, 4)
    case(call + "/id_plane mat float32", call, cur(mat=z(4, 4), prim_index=z(1)), None, cam, None, 4, id_plane="mat")
    case(call + "/id_plane None: the ids are not read", call, cur(prim_index=[1.0]), None, cam, None, 4, id_plane=None)
    case(call + "/another entry is ignored", call, cur(albedo=[1.0], motion=[1.0]), None, cam, None, 4)
    case(call + "/history a list", call, cur(), [1.0], cam, cam, 4)
    case(call + "/history float64", call, cur(), hist.to(f64), cam, cam, 4)
    case(call + "/history [3, 4, 4]", call, cur(), z(3, 4, 4), cam, cam, 4)
    case(call + "/history [4, 4, 4, 3]", call, cur(), z(4, 4, 4, 3), cam, cam, 4)
    case(call + "/history [3, 4, 4, 3]", call, cur(), z(3, 4, 4, 3), cam, cam, 4)
    case(call + "/history empty", call, cur(), z(3, 0, 4, 4), cam, cam, 4)
    case(call + "/history strided", call, cur(), z(3, 6, 2, 4).transpose(1, 2), cam, cam, 4)
    case(call + "/motion [4, 4]", call, cur(), None, cam, None, 4, motion=z(4, 4))
    case(call + "/motion int32", call, cur(), None, cam, None, 4, motion=z(4, 4, 3, dtype=i32))
    case(call + "/history without cam_prev", call, cur(), hist, cam, None, 4)
    case(call + "/cam_cur of three", call, cur(), None, (1.0, 2.0, 3.0), None, 4)
    case(call + "/cam_cur a float", call, cur(), None, 1.0, None, 4)
    case(call + "/cam_prev of three", call, cur(), hist, cam, (1.0, 2.0, 3.0), 4)
    case(call + "/cam_prev is not read without a history", call, cur(), None, cam, 1.0, 4)
    case(call + "/no cam_cur", call, cur(), None, None, None, 4)
    case(call + "/on the CPU", call, cur(normal=z(4, 4, 3), depth=z(4, 4), prim_index=z(4, 4, dtype=i32)), hist, cam, cam, 4, motion=z(4, 4, 3))
    case(call + "/n_colours 0 on the CPU", call, cur(), None, cam, None, 0)
    case(call + "/a camera of the wrong length on the CPU", call, cur(), None, ((0.0, 0.0), [0.0] * 16), None, 4)
    case(call + "/order: moments float64, depth a list", call, cur(moments=z(4, 4, 2, dtype=f64), depth=[1.0]), None, cam, None, 4)
    case(call + "/order: history float64 and [3, 4, 4]", call, cur(), z(3, 4, 4, dtype=f64), cam, cam, 4)
    case(call + "/order: history [3, 4, 4], no cam_prev", call, cur(), z(3, 4, 4), cam, None, 4)
    case(call + "/order: motion [4, 4], no cam_cur", call, cur(), None, None, None, 4, motion=z(4, 4))
    case(call + "/order: color on the CPU, no cam_cur", call, cur(), None, None, None, 4)
    case(call + "/order: color on the CPU, depth float64", call, cur(depth=z(4, 4, dtype=f64)), None, cam, None, 4)
    case(call + "/order: color on the CPU, motion a list", call, cur(), None, cam, None, 4, motion=[1.0])
    case(call + "/order: color float64, no moments", call, dict(color=z(4, 4, 3, dtype=f64)), None, cam, None, 4)

    case("temporal_camera/cam_pos of two", "temporal_camera", ((0.0, 0.0), [0.0] * 16), 4, 4)
    case("temporal_camera/cam_matrix of fifteen", "temporal_camera", ((0.0, 0.0, 0.0), [0.0] * 15), 4, 4)
    case("temporal_camera/cam_matrix [3, 4]", "temporal_camera", ((0.0, 0.0, 0.0), z(3, 4).numpy()), 4, 4)

    call = "svgf_spatial_variance_torch"
    case(call + "/width 0", call, z(3, 4, 4, 4), z(4, 4), 0, 4)
    case(call + "/height -1 before a bad tensor", call, [1.0], z(4, 4), 4, -1)
    case(call + "/hist a list", call, [1.0], z(4, 4), 4, 4)
    case(call + "/hist None", call, None, z(4, 4), 4, 4)
    case(call + "/variance None", call, z(3, 4, 4, 4), None, 4, 4)
    case(call + "/hist float64", call, z(3, 4, 4, 4, dtype=f64), z(4, 4), 4, 4)
    case(call + "/hist [3, 4, 5, 4] for 4 x 5", call, z(3, 4, 5, 4), z(5, 4), 4, 5)
    case(call + "/hist strided", call, z(3, 4, 4, 4).transpose(1, 2), z(4, 4), 4, 4)
    case(call + "/variance [4, 4, 1]", call, z(3, 4, 4, 4), z(4, 4, 1), 4, 4)
    case(call + "/variance int32", call, z(3, 4, 4, 4), z(4, 4, dtype=i32), 4, 4)
    case(call + "/out a list", call, z(3, 4, 4, 4), z(4, 4), 4, 4, out=[1.0])
    case(call + "/out [16]", call, z(3, 4, 4, 4), z(4, 4), 4, 4, out=z(16))
    case(call + "/out strided", call, z(3, 5, 4, 4), z(5, 4), 4, 5, out=z(4, 5).t())
    case(call + "/on the CPU", call, z(3, 5, 4, 4), z(5, 4), 4, 5, out=z(5, 4))
    case(call + "/out is variance on the CPU", call, z(3, 4, 4, 4), z(4, 4), 4, 4)
    case(call + "/order: hist float64, variance a list", call, z(3, 4, 4, 4, dtype=f64), [1.0], 4, 4)
    case(call + "/order: hist float64 and [3, 4, 4]", call, z(3, 4, 4, dtype=f64), z(4, 4), 4, 4)
    case(call + "/order: hist on the CPU, variance a list", call, z(3, 4, 4, 4), [1.0], 4, 4)
    case(call + "/order: hist on the CPU, out float64", call, z(3, 4, 4, 4), z(4, 4), 4, 4, out=z(4, 4, dtype=f64))

    # _frame_tensor through its three callers (the frame of the stub Backend is 4 x 4)
    call = "compact_mask_torch"
    case(call + "/mask a list", call, [1] * 16)
    case(call + "/mask None", call, None)
    case(call + "/mask uint8 on the CPU", call, z(4, 4, dtype=u8))
    case(call + "/mask bool on the CPU", call, z(16, dtype=torch.bool))
    case(call + "/order: mask float32 on the CPU", call, z(4, 4))
    case(call + "/order: mask too small on the CPU", call, z(15, dtype=u8))
    case(call + "/order: mask strided on the CPU", call, z(4, 8, dtype=u8)[:, ::2])
    call = "render_pass_masked"
    case(call + "/mask a list", call, P, 0, [1] * 16)
    case(call + "/mask bool on the CPU", call, P, 0, z(4, 4, dtype=torch.bool))
    case(call + "/order: mask on the CPU, counts a list", call, P, 0, z(4, 4, dtype=u8), [0] * 16)
    case(call + "/order: mask on the CPU, counts float32", call, P, 0, z(4, 4, dtype=u8), counts=z(4, 4))
    call = "adaptive_estimate_torch"
    case(call + "/accum a list", call, [0.0] * 48, z(4, 4, 2), z(4, 4, dtype=i32), True)
    case(call + "/accum None", call, None, None, None, True)
    case(call + "/on the CPU", call, z(4, 4, 3), z(4, 4, 2), z(4, 4, dtype=i32), True)
    case(call + "/order: accum float64 on the CPU", call, z(4, 4, 3, dtype=f64), z(4, 4, 2), z(4, 4, dtype=i32), False)
    case(call + "/order: accum too small on the CPU", call, z(47), z(4, 4, 2), z(4, 4, dtype=i32), False)
    case(call + "/order: accum on the CPU, moments a list", call, z(4, 4, 3), [1.0], z(4, 4, dtype=i32), False)
    case(call + "/order: accum on the CPU, an unknown plane", call, z(4, 4, 3), z(4, 4, 2), z(4, 4, dtype=i32), False, want=("nope",))
    case(call + "/order: accum on the CPU, no plane", call, z(4, 4, 3), z(4, 4, 2), z(4, 4, dtype=i32), False, want=())

    for call, first in (("refit_torch", ()), ("rebuild_torch", ()), ("refit_mesh_torch", (0,))):
        case(call + "/pos a list", call, *first, [[0.0, 0.0, 0.0]])
        case(call + "/pos 1-D", call, *first, z(6))
        case(call + "/pos float64", call, *first, z(4, 3, dtype=f64))
        case(call + "/pos [4, 2]", call, *first, z(4, 2))
        case(call + "/nrm a list", call, *first, z(4, 3), [1.0])
        case(call + "/nrm float64", call, *first, z(4, 3), z(4, 3, dtype=f64))
        case(call + "/nrm [5, 3]", call, *first, z(4, 3), z(5, 3))
        case(call + "/on the CPU", call, *first, z(4, 3), z(4, 3))
        case(call + "/strided on the CPU", call, *first, z(3, 4).t())
        case(call + "/no vertices on the CPU", call, *first, z(0, 3))
        case(call + "/order: pos float64, nrm a list", call, *first, z(4, 3, dtype=f64), [1.0])
        case(call + "/order: pos float64 and [4, 2]", call, *first, z(4, 2, dtype=f64))
        case(call + "/order: pos on the CPU, nrm [5, 3]", call, *first, z(4, 3), z(5, 3))
    case("refit_torch/check=False on the CPU", "refit_torch", z(4, 3), check=False)

    case("set_camera/cam_pos of two", "set_camera", (0.0, 0.0))
    case("set_camera/cam_matrix of fifteen", "set_camera", (0.0, 0.0, 0.0), [0.0] * 15)
    case("set_camera/cam_matrix [3, 4]", "set_camera", (0.0, 0.0, 0.0), z(3, 4).numpy())

    call = "move_instances_torch"
    case(call + "/m a list", call, [[0.0] * 12])
    case(call + "/m float64", call, z(2, 12, dtype=f64))
    case(call + "/m [2, 11]", call, z(2, 11))
    case(call + "/m [2, 4, 3]", call, z(2, 4, 3))
    case(call + "/m 1-D", call, z(24))
    case(call + "/m [2, 12] on the CPU", call, z(2, 12))
    case(call + "/m [2, 3, 4] on the CPU", call, z(2, 3, 4))
    case(call + "/m strided on the CPU", call, z(12, 2).t())
    case(call + "/no instances on the CPU", call, z(0, 12))
    case(call + "/check=False on the CPU", call, z(2, 12), check=False)
    case(call + "/order: m float64 and [2, 11]", call, z(2, 11, dtype=f64))
    assert len(set(c[0] for c in table)) == len(table), "two cases share an id"
    return table


def refusal(art, ident, method, args, kwargs, attrs):
    """{"type", "message"} of what the case raises; a case that raises nothing, or reaches the library, is an error of the table"""
    be = stub_backend(art, attrs)
    try:
        getattr(be, method)(*args, **kwargs)
    except AssertionError:
        raise AssertionError("%s: nothing was refused: the library was called" % ident)
    except Exception as e:
        return {"type": type(e).__name__, "message": str(e)}
    raise AssertionError("%s: nothing was refused" % ident)


def surface(art):
    """the signatures of Backend's public methods and of SceneDesc.__init__; the module's public names that are not imported modules"""
    sigs = {}
    for name, f in sorted(vars(art.Backend).items()):
        f = f.__func__ if isinstance(f, staticmethod) else f
        if callable(f) and (not name.startswith("_") or name == "__init__"):
            sigs["Backend." + name] = str(inspect.signature(f))
    sigs["SceneDesc.__init__"] = str(inspect.signature(art.SceneDesc.__init__))
    names = sorted(name for name, v in vars(art).items() if not name.startswith("_") and not isinstance(v, types.ModuleType))
    return sigs, names


def record(art, torch):
    sigs, names = surface(art)
    return {"refusals": {c[0]: refusal(art, *c) for c in cases(art, torch)}, "signatures": sigs, "public_names": names}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_refusal_is_the_recorded_one(art):
    import torch
    want = golden()["refusals"]
    table = cases(art, torch)
    assert [c[0] for c in table] == list(want), "the table and the record hold different cases"
    got = {c[0]: refusal(art, *c) for c in table}
    wrong = ["%s:\n    recorded %s(%r)\n    raised   %s(%r)" % (k, want[k]["type"], want[k]["message"], got[k]["type"], got[k]["message"])
             for k in want if got[k] != want[k]]
    assert not wrong, "%d of %d refusals differ from the record:\n%s" % (len(wrong), len(want), "\n".join(wrong))


def test_the_table_reaches_every_wrapper_and_every_kind_of_refusal(art):
    """a guard of the table itself: the wrappers the record must cover are all there, with more than the first refusal of each"""
    want = golden()["refusals"]
    methods = collections.Counter(k.split("/")[0] for k in want)
    for name in ("resize", "bind_accum", "bind_moments", "trace_rays_torch", "occluded_torch", "render_aovs_torch", "render_aovs_torch_motion",
                 "denoise_torch", "denoise_svgf_torch", "temporal_torch", "temporal_camera", "svgf_spatial_variance_torch", "compact_mask_torch",
                 "render_pass_masked", "adaptive_estimate_torch", "refit_torch", "rebuild_torch", "refit_mesh_torch", "set_camera",
                 "move_instances_torch"):
        assert methods[name] >= 1, name
    texts = " ".join(v["message"] for v in want.values())
    for words in ("a torch tensor is required", "dtype must be", "the tensor must be contiguous", "must be a GPU tensor", "shape must be",
                  "expected", "must hold at least", "the bound accum tensor holds", "the bound moments tensor holds", "unknown plane",
                  "unexpected keyword argument", "not both", "a history needs the camera", "a camera is (cam_pos, cam_matrix)",
                  "a dict of planes is required", "width and height must be at least 1", "cam_pos takes 3 floats",
                  "a [N, 3] float32 tensor is required", "a [nverts, 3] float32 tensor is required",
                  "None, an integer device address or a torch tensor is required"):
        assert words in texts, words
    assert set(v["type"] for v in want.values()) == {"ArtError", "ValueError", "TypeError"}


def test_signatures_and_public_names_are_the_recorded_ones(art):
    want = golden()
    sigs, names = surface(art)
    assert sigs == want["signatures"]
    assert names == want["public_names"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_python_refusals.py --record")
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    import __graft_entry__ as ge
    with open(GOLDEN, "w") as f:
        json.dump(record(ge.load_package(), torch), f, indent=1, sort_keys=False)
        f.write("\n")
    print("recorded %s" % GOLDEN)
