"""Firefly suppression ahead of temporal accumulation (art_firefly_device; include/art_hip.h states the arithmetic): the parameter struct
of the C entry, the defaults and the torch-facing method, which Backend inherits.  The package's one tensor check, its device check and
its error type are the package's own: they are looked up when a method runs, so this module imports nothing of the package while the
package is being imported."""
import ctypes as C
import sys

# the defaults of firefly_torch: the best setting of the sweep of profiles/firefly/quality.py (quality.json, README.md beside it)
FIREFLY_RADIUS = 2
FIREFLY_RANK = 1
FIREFLY_GAIN = 8.0
FIREFLY_FLOOR = 0.05


class ArtFireflyParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("radius", C.c_int32), ("rank", C.c_int32), ("min_count", C.c_int32),
                ("scale", C.c_float), ("gain", C.c_float), ("floor", C.c_float)]


class FireflyCalls:
    """What Backend gains: firefly_torch (self.lib is the loaded library)."""

    def firefly_torch(self, color, moments=None, id=None, out=None, moments_out=None, radius=FIREFLY_RADIUS, rank=FIREFLY_RANK, min_count=None,
                      scale=1.0, gain=FIREFLY_GAIN, floor=FIREFLY_FLOOR):
        """Outliers taken out of a frame before temporal_torch (art_firefly_device; include/art_hip.h states the arithmetic): a pixel
        whose luminance exceeds gain * (the rank-th largest luminance among its neighbours within `radius`) + floor is scaled down to
        that limit, and its moments with it.  color: float32 [H, W, 3] (the tensor of bind_accum is accepted as it is, scale = 1 / spp);
        moments: None or float32 with at least 2 * H * W elements (the tensor of bind_moments as it is); id: None or int32 [H, W] (e.g.
        render_aovs_torch's prim_index): only neighbours of the pixel's own id count.  min_count: a pixel with fewer neighbours is left
        alone; None = rank.  out: None (a new tensor) or float32 [H, W, 3], which may be `color` itself; moments_out: likewise for the
        moments, it may be `moments` itself.  Returns (out, moments_out, clamped): out holds the SCALED colour (what follows takes
        scale = 1), moments_out is None without moments, clamped is uint8 [H, W]: 0 kept, 1 clamped, 2 not finite -- what
        compact_mask_torch takes.  Enqueued on torch.cuda.current_stream() without waiting for it.  Every tensor is checked before any
        C call."""
        from . import ArtError, _check, _check_devices, _check_planes, _colour_frame, _handle, _image_plane, _ptr, _stream
        torch = sys.modules.get("torch")
        call = "firefly_torch"
        h, w = _colour_frame(torch, call, color)
        if moments is None and moments_out is not None:
            raise ArtError("%s: moments_out is given without moments" % call)
        planes = [_image_plane(call, h, w, "color", color, 3, optional=False), _image_plane(call, h, w, "moments", moments, 2),
                  _image_plane(call, h, w, "id", id, 1, "int32"), _image_plane(call, h, w, "out", out, 3),
                  _image_plane(call, h, w, "moments_out", moments_out, 2)]
        _check_planes(torch, planes)
        _check_devices(planes, color.device)
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=color.device)
        if moments is not None and moments_out is None:
            moments_out = torch.empty((h, w, 2), dtype=torch.float32, device=color.device)
        clamped = torch.empty((h, w), dtype=torch.uint8, device=color.device)
        p = ArtFireflyParams(w, h, int(radius), int(rank), int(rank if min_count is None else min_count), float(scale), float(gain), float(floor))
        _check(self.lib.art_firefly_device(C.byref(p), color.data_ptr(), _ptr(moments), _ptr(id), out.data_ptr(), _ptr(moments_out), clamped.data_ptr(),
                                           _handle(_stream(torch, color.device))))
        return out, moments_out, clamped
