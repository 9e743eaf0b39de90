"""Feature buffers along the caller's rays and the frame's camera rays (art_aovs_rays_device, art_camera_rays_device; include/art_hip.h
states the contract): the structs of the C entries and the torch-facing methods, which Backend inherits.  The package's one tensor check,
its device check and its error type are the package's own: they are looked up when a method runs, so this module imports nothing of the
package while the package is being imported."""
import collections
import ctypes as C
import numbers
import sys


class ArtAovRaysParams(C.Structure):
    _fields_ = [("group", C.c_int32), ("background", C.c_float * 3)]


class ArtAovRayBuffers(C.Structure):
    _fields_ = [("albedo3f", C.c_void_p), ("normal3f", C.c_void_p), ("position3f", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p),
                ("prim_type", C.c_void_p), ("prim_index", C.c_void_p), ("mat", C.c_void_p)]


# aovs_rays_torch: plane -> (field of ArtAovRayBuffers, floats or ints per group, integer plane)
RAY_PLANES = collections.OrderedDict([("albedo", ("albedo3f", 3, False)), ("normal", ("normal3f", 3, False)), ("position", ("position3f", 3, False)),
                                      ("depth", ("depth", 1, False)), ("alpha", ("alpha", 1, False)), ("prim_type", ("prim_type", 1, True)),
                                      ("prim_index", ("prim_index", 1, True)), ("mat", ("mat", 1, True))])
MAX_GROUP = 16


class AovRayCalls:
    """What Backend gains: aovs_rays_torch and camera_rays_torch (self.lib is the loaded library)."""

    def aovs_rays_torch(self, origins, dirs, group=1, tnear=None, tfar=None, background=(0.0, 0.0, 0.0), want=tuple(RAY_PLANES), out=None):
        """First-hit feature buffers along N rays held in torch tensors on the GPU (art_aovs_rays_device; include/art_hip.h states the
        contract).  origins, dirs: [N, 3] float32 (dirs are used as given, not normalised); tnear, tfar: [N] float32 or None.  Rays are
        group-major: element g of a plane owns rays g * group .. g * group + group - 1 (group 1..16, N a multiple of it), a float
        plane holds their mean in the header's association, an id plane ray 0's.  Returns a dict of tensors on the rays' device, one
        per name in `want` -- albedo, normal, position [N // group, 3] float32; depth, alpha [N // group] float32; prim_type,
        prim_index, mat [N // group] int32 -- new tensors, or those of the dict `out` (name -> tensor, contiguous; a name outside
        `want` is refused).  An unknown name raises ValueError.  Every tensor is checked before any C call; the call is enqueued on
        torch.cuda.current_stream() without waiting for it."""
        from . import ArtError, _Plane, _check, _check_devices, _check_planes, _expected, _handle, _ptr, _stream
        torch = sys.modules.get("torch")
        call = "aovs_rays_torch"
        want = tuple(want)
        for name in want + tuple(out or ()):
            if name not in RAY_PLANES:
                raise ValueError("%s: unknown plane %r (known: %s)" % (call, name, ", ".join(RAY_PLANES)))
        if not want:
            raise ArtError("%s: want: at least one plane" % call)
        for name in (out or ()):
            if name not in want:
                raise ArtError("%s: out: plane %r is not in want" % (call, name))
        if not isinstance(group, numbers.Integral) or isinstance(group, bool) or group < 1 or group > MAX_GROUP:
            raise ArtError("%s: group must be an integer 1..%d, not %r" % (call, MAX_GROUP, group))
        if torch is None or not isinstance(origins, torch.Tensor) or origins.dim() != 2:
            raise ArtError("%s: origins: a [N, 3] float32 tensor is required" % call)
        group, n = int(group), int(origins.shape[0])
        if n % group:
            raise ArtError("%s: %d rays are not a multiple of group %d" % (call, n, group))
        g = n // group
        if len(tuple(background)) != 3:
            raise ArtError("%s: background takes 3 floats" % call)
        inputs = [_Plane(call + ": origins", origins, "float32", _expected(n, 3)), _Plane(call + ": dirs", dirs, "float32", _expected(n, 3)),
                  _Plane(call + ": tnear", tnear, "float32", _expected(n), True), _Plane(call + ": tfar", tfar, "float32", _expected(n), True)]
        outputs = [_Plane("%s: out[%r]" % (call, name), x, "int32" if RAY_PLANES[name][2] else "float32",
                          _expected(g, 3) if RAY_PLANES[name][1] == 3 else _expected(g)) for name, x in (out or {}).items()]
        o, d, tn, tf = _check_planes(torch, inputs, "make")
        _check_planes(torch, outputs)
        _check_devices(inputs + outputs, o.device)
        planes, buf = {}, ArtAovRayBuffers()
        for name in want:
            field, per, integer = RAY_PLANES[name]
            x = (out or {}).get(name)
            if x is None:
                x = torch.empty((g, 3) if per == 3 else (g,), dtype=torch.int32 if integer else torch.float32, device=o.device)
            planes[name] = x
            setattr(buf, field, x.data_ptr() or None)
        p = ArtAovRaysParams(group, (C.c_float * 3)(*[float(v) for v in background]))
        _check(self.lib.art_aovs_rays_device(C.byref(p), _ptr(o) if n else None, _ptr(d) if n else None, _ptr(tn) if n else None,
                                             _ptr(tf) if n else None, n, C.byref(buf), _handle(_stream(torch, o.device))))
        return planes

    def camera_rays_torch(self, params):
        """The frame's camera rays (art_camera_rays_device): (origins, dirs), float32 [H * W * K, 3] on torch's current GPU, K = 4 with
        params.aa_on, else 1; ray s of pixel y * W + x is row (y * W + x) * K + s: cam_pos and the direction a render pass traces for that
        sample.  Of `params` only aa_on is read.  Fed to aovs_rays_torch with group = K they give render_aovs_torch's planes.  Enqueued on
        torch.cuda.current_stream() without waiting for it."""
        from . import _check, _handle, _stream
        torch = sys.modules.get("torch") or __import__("torch")
        dev = torch.device("cuda", torch.cuda.current_device())
        n = int(getattr(self, "height", 0)) * int(getattr(self, "width", 0)) * (4 if params.aa_on else 1)
        o = torch.empty((n, 3), dtype=torch.float32, device=dev)
        d = torch.empty((n, 3), dtype=torch.float32, device=dev)
        _check(self.lib.art_camera_rays_device(C.byref(params), o.data_ptr() or None, d.data_ptr() or None, _handle(_stream(torch, dev))))
        return o, d
