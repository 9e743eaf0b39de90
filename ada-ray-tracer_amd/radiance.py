"""Radiance queries (art_radiance_rays_device; include/art_hip.h states the contract): the parameter struct of the C entry and the
torch-facing method, which Backend inherits.  The package's one tensor check, its device check and its error type are the package's
own: they are looked up when the method runs, so this module imports nothing of the package while the package is being imported."""
import ctypes as C
import sys

PT_MIS = 4      # ray_tracer.ads:40, as in the package


class ArtRadianceParams(C.Structure):
    _fields_ = [("render_type", C.c_int32), ("max_depth", C.c_int32), ("samples", C.c_int32), ("sample_base", C.c_uint32), ("seed", C.c_uint64)]


class RadianceQueries:
    """What Backend gains: radiance_rays_torch (self.lib is the loaded library)."""

    def radiance_rays_torch(self, origins, dirs, *, render_type=PT_MIS, max_depth=8, samples=1, sample_base=0, seed=1, keys=None, out=None,
                            moments=None):
        """Radiance along N rays held in torch tensors on the GPU (art_radiance_rays_device; include/art_hip.h states the contract):
        `samples` paths per ray with the integrator render_type selects, RNG keyed by (seed, keys[i] or i, sample_base + k, bounce).
        origins, dirs: [N, 3] float32 (dirs are used as given, not normalised); keys: None or [N] int32 (uint32 words).  Returns the
        [N, 3] float32 sum of the path values on the rays' device: a new zeroed tensor, or `out` ([N, 3] float32), into which the
        call accumulates; moments ([N, 2] float32, optional) takes the luminance sums {S1, S2} the same way.  Tensors are checked
        before any C call; out and moments must be contiguous, the inputs are made so.  The library works on its own stream and the
        call waits for it; what torch's current stream still has in flight (the producers of the inputs) is waited for first."""
        from . import ArtError, _Plane, _check, _check_devices, _check_planes, _expected, _ptr
        torch = sys.modules.get("torch")
        call = "radiance_rays_torch"
        if torch is None or not isinstance(origins, torch.Tensor) or origins.dim() != 2:
            raise ArtError("%s: origins: a [N, 3] float32 tensor is required" % call)
        n = int(origins.shape[0])
        inputs = [_Plane(call + ": origins", origins, "float32", _expected(n, 3)), _Plane(call + ": dirs", dirs, "float32", _expected(n, 3)),
                  _Plane(call + ": keys", keys, "int32", _expected(n), True)]
        outputs = [_Plane(call + ": out", out, "float32", _expected(n, 3), True), _Plane(call + ": moments", moments, "float32", _expected(n, 2), True)]
        o, d, k = _check_planes(torch, inputs, "make")
        _check_planes(torch, outputs)
        _check_devices(inputs + outputs, o.device)
        if out is None:
            out = torch.zeros((n, 3), dtype=torch.float32, device=o.device)
        torch.cuda.current_stream(o.device).synchronize()      # the header's rule: inputs written on another stream are complete before the call
        p = ArtRadianceParams(int(render_type), int(max_depth), int(samples), int(sample_base), int(seed))
        _check(self.lib.art_radiance_rays_device(C.byref(p), _ptr(o) if n else None, _ptr(d) if n else None, _ptr(k) if n else None, n,
                                                 out.data_ptr() if n else None, _ptr(moments) if n else None))
        return out
