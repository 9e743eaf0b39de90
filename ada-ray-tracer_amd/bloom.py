"""Bloom ahead of the display transform (art_bloom_device; include/art_hip.h states the arithmetic): the parameter struct of the C entry,
the defaults and the torch-facing method, which Backend inherits.  The package's one tensor check, its device check and its error type
are the package's own: they are looked up when a method runs, so this module imports nothing of the package while the package is being
imported."""
import ctypes as C
import sys

# The defaults of bloom_torch are conventional values, a matter of taste and NOT the result of a sweep: bloom is not an estimator, so
# there is no error a setting could minimise.  Threshold and knee 0: every pixel scatters, which conserves energy.
BLOOM_LEVELS = 6
BLOOM_SCATTER = 0.7
BLOOM_STRENGTH = 0.05
BLOOM_THRESHOLD = 0.0
BLOOM_KNEE = 0.0
BLOOM_KARIS = 1
# 0: the small levels in one workgroup (the tail kernel); 1: one launch per level.  The same words either way.  The default follows
# profiles/bloom/measure.json (README.md beside it): at the default six levels the tail does not beat the per-level route (0.0760 against
# 0.0756 ms at 1920 x 1080), so that route is the default; at eight levels it does (0.080 against 0.091 ms): pass variant=0 there.
BLOOM_VARIANT = 1
STATE_WORDS = 4 + 256       # the exposure state of auto_exposure_torch (include/art_hip.h)


class ArtBloomParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32), ("karis", C.c_int32), ("variant", C.c_int32),
                ("scale", C.c_float), ("exposure", C.c_float), ("threshold", C.c_float), ("knee", C.c_float), ("scatter", C.c_float),
                ("strength", C.c_float)]


class BloomCalls:
    """What Backend gains: bloom_torch (self.lib is the loaded library)."""

    def bloom_torch(self, color, exposure_state=None, out=None, bloom_out=None, levels=BLOOM_LEVELS, karis=BLOOM_KARIS, variant=BLOOM_VARIANT,
                    scale=1.0, exposure=1.0, threshold=BLOOM_THRESHOLD, knee=BLOOM_KNEE, scatter=BLOOM_SCATTER, strength=BLOOM_STRENGTH,
                    want_out=True, want_bloom=True):
        """The glare of bright pixels mixed into a frame (art_bloom_device; include/art_hip.h states the arithmetic): the frame is
        filtered down a pyramid of `levels` halved levels, the levels are blended back up with `scatter`, and the result B is mixed in:
        out = s + strength * (B - s), s the sanitised scale * color.  color: float32 [H, W, 3] (the tensor of bind_accum is accepted
        as it is, scale = 1 / spp); exposure_state: the tensor of auto_exposure_torch or None for `exposure` -- only a threshold or a
        knee that is not 0 reads it.  out: None (a new tensor) or float32 [H, W, 3], which may be `color` itself; bloom_out: likewise
        for B alone (it may not be `color`).  want_out / want_bloom = False leaves that plane out (not both).  Returns (out, bloom),
        a plane left out as None; out holds the SCALED colour (what follows takes scale = 1).  Enqueued on torch.cuda.current_stream()
        without waiting for it.  Every tensor is checked before any C call."""
        from . import ArtError, _Plane, _check, _check_devices, _check_planes, _colour_frame, _handle, _image_plane, _ptr, _stream
        torch = sys.modules.get("torch")
        call = "bloom_torch"
        h, w = _colour_frame(torch, call, color)
        planes = [_image_plane(call, h, w, "color", color, 3, optional=False), _Plane(call + ": exposure_state", exposure_state, "int32", (STATE_WORDS,), True),
                  _image_plane(call, h, w, "out", out, 3), _image_plane(call, h, w, "bloom_out", bloom_out, 3)]
        _check_planes(torch, planes)
        _check_devices(planes, color.device)
        if not want_out and not want_bloom:
            raise ArtError("%s: neither out nor bloom is wanted" % call)
        if (not want_out and out is not None) or (not want_bloom and bloom_out is not None):
            raise ArtError("%s: a plane is given that want_out / want_bloom = False leaves out" % call)
        if want_out and out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=color.device)
        if want_bloom and bloom_out is None:
            bloom_out = torch.empty((h, w, 3), dtype=torch.float32, device=color.device)
        p = ArtBloomParams(w, h, int(levels), int(karis), int(variant), float(scale), float(exposure), float(threshold), float(knee), float(scatter),
                           float(strength))
        _check(self.lib.art_bloom_device(C.byref(p), color.data_ptr(), _ptr(exposure_state), _ptr(out), _ptr(bloom_out), _handle(_stream(torch, color.device))))
        return out, bloom_out
