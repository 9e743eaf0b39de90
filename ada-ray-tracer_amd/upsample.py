"""Guided upsampling of a low-resolution render (art_upsample_device; include/art_hip.h states the arithmetic): the parameter structs of
the C entry and the torch-facing method, which Backend inherits.  The package's one tensor check, its device check and its error type are
the package's own: they are looked up when a method runs, so this module imports nothing of the package while the package is being
imported."""
import ctypes as C
import sys

GUIDES = ("albedo", "normal", "depth", "id")
UPSAMPLE_SIGMA_DEPTH = 4.0      # the defaults of upsample_torch: the best of the sweep of profiles/upsample/quality.py (quality.json)
UPSAMPLE_NORMAL_LOG2 = 5


class ArtUpsampleParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("lo_width", C.c_int32), ("lo_height", C.c_int32), ("footprint", C.c_int32),
                ("demodulate", C.c_int32), ("normal_log2", C.c_int32), ("scale", C.c_float), ("sigma_depth", C.c_float), ("jitter", C.c_float * 2)]


class ArtUpsampleGuides(C.Structure):
    _fields_ = [("albedo3f", C.c_void_p), ("normal3f", C.c_void_p), ("depth", C.c_void_p), ("id", C.c_void_p)]


class UpsampleCalls:
    """What Backend gains: upsample_torch (self.lib is the loaded library)."""

    def upsample_torch(self, lo_color, lo_guides, hi_guides, footprint=2, scale=1.0, sigma_depth=UPSAMPLE_SIGMA_DEPTH, normal_log2=UPSAMPLE_NORMAL_LOG2,
                       jitter=(0.0, 0.0), demodulate=True, want_fallback=False, out=None):
        """A lo colour plane as a hi picture under feature buffers at both resolutions (art_upsample_device; include/art_hip.h states the
        arithmetic).  lo_color: float32 [LH, LW, 3] (the tensor of bind_accum at the lo viewport is accepted as it is, scale = 1 / spp).
        lo_guides, hi_guides: dicts with the keys albedo, normal (float32 [.., .., 3]), depth (float32 [.., ..]) and id (int32 [.., ..],
        e.g. render_aovs_torch's prim_index), each absent or None on both sides or given on both; other keys (the rest of
        render_aovs_torch's dict) are ignored.  The hi frame's size is that of a hi guide, or of `out`, or with neither the lo frame's.
        demodulate: divide by the lo albedo and multiply by the hi albedo where albedo is given.  Returns out, float32 [H, W, 3] (out:
        that tensor, or None for a new one), or (out, fallback) with want_fallback: a uint8 [H, W] tensor, 0 where the guides
        reconstructed the pixel, 1 unguided, 2 black -- what compact_mask_torch takes.  Enqueued on torch.cuda.current_stream() without
        waiting for it.  Every tensor is checked before any C call."""
        from . import ArtError, _Plane, _check, _check_devices, _check_planes, _colour_frame, _handle, _image_plane, _ptr, _stream
        torch = sys.modules.get("torch")
        call = "upsample_torch"
        lh, lw = _colour_frame(torch, call, lo_color)
        for side, g in (("lo_guides", lo_guides), ("hi_guides", hi_guides)):
            if not isinstance(g, dict):
                raise ArtError("%s: %s: a dict of planes is required, not %s" % (call, side, type(g).__name__))
        lo = {k: lo_guides.get(k) for k in GUIDES}
        hi = {k: hi_guides.get(k) for k in GUIDES}
        for k in GUIDES:
            if (lo[k] is None) != (hi[k] is None):
                raise ArtError("%s: %s is given on one side only (lo_guides and hi_guides must hold the same planes)" % (call, k))
        first = next((x for x in list(hi.values()) + [out] if x is not None), None)
        if first is not None and not (torch is not None and isinstance(first, torch.Tensor) and first.dim() >= 2):
            raise ArtError("%s: hi_guides: a torch tensor [H, W, ..] is required, not %s" % (call, type(first).__name__))
        h, w = (int(first.shape[0]), int(first.shape[1])) if first is not None else (lh, lw)
        per = {"albedo": (3, "float32"), "normal": (3, "float32"), "depth": (1, "float32"), "id": (1, "int32")}
        planes = [_image_plane(call, lh, lw, "lo_color", lo_color, 3, optional=False)]
        planes += [_image_plane(call, lh, lw, "lo_guides[%r]" % k, lo[k], *per[k]) for k in GUIDES]
        planes += [_image_plane(call, h, w, "hi_guides[%r]" % k, hi[k], *per[k]) for k in GUIDES]
        planes.append(_image_plane(call, h, w, "out", out, 3))
        _check_planes(torch, planes)
        _check_devices(planes, lo_color.device)
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=lo_color.device)
        fallback = torch.empty((h, w), dtype=torch.uint8, device=lo_color.device) if want_fallback else None
        p = ArtUpsampleParams(w, h, lw, lh, int(footprint), 1 if (demodulate and lo["albedo"] is not None) else 0, int(normal_log2), float(scale),
                              float(sigma_depth), (C.c_float * 2)(float(jitter[0]), float(jitter[1])))
        gl = ArtUpsampleGuides(*[_ptr(lo[k]) for k in GUIDES])
        gh = ArtUpsampleGuides(*[_ptr(hi[k]) for k in GUIDES])
        _check(self.lib.art_upsample_device(C.byref(p), lo_color.data_ptr(), C.byref(gl), C.byref(gh), out.data_ptr(), _ptr(fallback),
                                            _handle(_stream(torch, lo_color.device))))
        return (out, fallback) if want_fallback else out
