"""Temporal super-resolution (art_temporal_upsample_device; include/art_hip.h states the arithmetic): jittered low-resolution frames
accumulated into a full-resolution history.  The parameter structs of the C entry, the torch-facing method, which Backend inherits, the
jitter sequence and the camera that traces a jittered lo grid.  The package's one tensor check, its device check and its error type are
the package's own: they are looked up when a method runs, so this module imports nothing of the package while the package is being
imported."""
import ctypes as C
import sys

import numpy as np

GUIDES = ("normal", "depth", "id")
# the defaults of temporal_upsample_torch: the best of the sweep of profiles/temporal_upsample/quality.py (quality.json)
TEMPORAL_UPSAMPLE_RADIUS = 1.5              # in hi pixels; cut to min(W / LW, H / LH) where that is smaller
TEMPORAL_UPSAMPLE_MIN_CONFIDENCE = 0.0078125


class ArtTemporalUpsampleGuides(C.Structure):
    _fields_ = [("normal3f", C.c_void_p), ("depth", C.c_void_p), ("id", C.c_void_p), ("motion3f", C.c_void_p)]


def _params_struct():
    from . import ArtTemporalParams

    class ArtTemporalUpsampleParams(C.Structure):
        _fields_ = [("t", ArtTemporalParams), ("lo_width", C.c_int32), ("lo_height", C.c_int32), ("jitter", C.c_float * 2), ("radius", C.c_float),
                    ("min_confidence", C.c_float)]
    return ArtTemporalUpsampleParams


_struct = None


def params_struct():
    """ArtTemporalUpsampleParams (it embeds the package's ArtTemporalParams, so it is made when first asked for)"""
    global _struct
    if _struct is None:
        _struct = _params_struct()
    return _struct


def _halton(i, base):
    f, r = 1.0, 0.0
    while i > 0:
        f /= base
        r += f * (i % base)
        i //= base
    return r


def jitter_sequence(n):
    """n jitters [n, 2] float32: the Halton points of bases (2, 3) from index 1, minus 0.5, clipped inside the open interval (-0.5, 0.5)"""
    lim = np.float32(0.5) - np.float32(2.0 ** -10)
    j = np.array([[_halton(i + 1, 2) - 0.5, _halton(i + 1, 3) - 0.5] for i in range(int(n))], np.float64).reshape(-1, 2)
    return np.clip(j, -lim, lim).astype(np.float32)


def jittered_camera(cam_matrix, lo_width, jitter):
    """The cam_matrix (16 floats or [4, 4], row-major) under which a render pass at a viewport lo_width wide traces the lo grid moved by
    jitter (jx, jy) lo pixels: camera_dir is normalize(M normalize(r)) with r.z = cam_z = -lo_width, so moving r by (jx, jy, 0) is the
    shear M'[k][2] = M[k][2] + (jx * M[k][0] + jy * M[k][1]) / cam_z.  The translation column stays as it is (zero).  Returns float32
    [4, 4] for set_camera."""
    m = np.array(cam_matrix, np.float64).reshape(4, 4)
    cam_z = -float(lo_width)
    out = m.copy()
    out[:3, 2] = m[:3, 2] + (float(jitter[0]) * m[:3, 0] + float(jitter[1]) * m[:3, 1]) / cam_z
    return out.astype(np.float32)


class TemporalUpsampleCalls:
    """What Backend gains: temporal_upsample_torch (self.lib is the loaded library)."""

    def temporal_upsample_torch(self, lo_color, lo_moments, lo, hi, cur, prev=None, hist_in=None, jitter=(0.0, 0.0), n_colours=1, scale=1.0,
                                radius=None, min_confidence=TEMPORAL_UPSAMPLE_MIN_CONFIDENCE, max_history=None, depth_tol=None, normal_min=None,
                                size=None, want_fallback=False):
        """One jittered lo frame into the hi history (art_temporal_upsample_device; include/art_hip.h states the arithmetic).  lo_color:
        float32 [LH, LW, 3] and lo_moments: float32 with 2 * LH * LW elements (the tensors of bind_accum and bind_moments at the lo
        viewport, scale = 1 / spp, n_colours as in temporal_torch).  lo, hi: dicts with the keys normal (float32 [.., .., 3]), depth
        (float32 [.., ..]) and id (int32 [.., ..]), each absent or None on both sides or given on both -- lo traced with the jittered
        camera, hi with the unjittered one; hi may also hold motion (float32 [H, W, 3], render_aovs_torch_motion's plane); other keys
        are ignored.  cur, prev: (cam_pos, cam_matrix), the UNJITTERED cameras of this frame and of hist_in's (prev is not read without
        hist_in).  hist_in: the history of the previous call, float32 [3, H', W', 4], or None.  jitter: this frame's, in lo pixels.
        The hi frame's size is that of a hi plane, or `size` = (W, H), or with neither the lo frame's.  radius None: the swept default
        TEMPORAL_UPSAMPLE_RADIUS, cut to min(W / LW, H / LH); max_history, depth_tol, normal_min None: temporal_torch's defaults.
        Returns (out [H, W, 3], variance [H, W], length [H, W], hist_out [3, H, W, 4]), float32, and with want_fallback a fifth, uint8
        [H, W] -- what compact_mask_torch takes.  Enqueued on torch.cuda.current_stream() without waiting for it.  Every tensor is
        checked before any C call."""
        from . import (ArtError, TEMPORAL_DEPTH_TOL, TEMPORAL_MAX_HISTORY, TEMPORAL_NORMAL_MIN, _Plane, _check, _check_devices, _check_planes, _colour_frame,
                       _handle, _image_plane, _ptr, _stream)
        torch = sys.modules.get("torch")
        call = "temporal_upsample_torch"
        lh, lw = _colour_frame(torch, call, lo_color)
        for side, g in (("lo", lo), ("hi", hi)):
            if not isinstance(g, dict):
                raise ArtError("%s: %s: a dict of planes is required, not %s" % (call, side, type(g).__name__))
        if lo.get("motion") is not None:
            raise ArtError("%s: lo: motion is the hi frame's plane (lo must not hold one)" % call)
        gl = {k: lo.get(k) for k in GUIDES}
        gh = {k: hi.get(k) for k in GUIDES}
        motion = hi.get("motion")
        for k in GUIDES:
            if (gl[k] is None) != (gh[k] is None):
                raise ArtError("%s: %s is given on one side only (lo and hi must hold the same planes)" % (call, k))
        first = next((x for x in list(gh.values()) + [motion] if x is not None), None)
        if first is not None and not (torch is not None and isinstance(first, torch.Tensor) and first.dim() >= 2):
            raise ArtError("%s: hi: a torch tensor [H, W, ..] is required, not %s" % (call, type(first).__name__))
        if first is not None:
            h, w = int(first.shape[0]), int(first.shape[1])
        elif size is not None:
            w, h = int(size[0]), int(size[1])
        else:
            h, w = lh, lw
        per = {"normal": (3, "float32"), "depth": (1, "float32"), "id": (1, "int32")}
        whole = (lambda x: x.dim() == 4 and x.shape[0] == 3 and x.shape[3] == 4 and x.numel() != 0, "shape must be [3, H', W', 4], not {}")
        planes = [_image_plane(call, lh, lw, "lo_color", lo_color, 3, optional=False), _image_plane(call, lh, lw, "lo_moments", lo_moments, 2, optional=False)]
        planes += [_image_plane(call, lh, lw, "lo[%r]" % k, gl[k], *per[k]) for k in GUIDES]
        planes += [_image_plane(call, h, w, "hi[%r]" % k, gh[k], *per[k]) for k in GUIDES]
        planes += [_image_plane(call, h, w, "hi['motion']", motion, 3), _Plane(call + ": hist_in", hist_in, "float32", whole, True)]
        _check_planes(torch, planes)
        if hist_in is not None and prev is None:
            raise ArtError("%s: prev: a history needs the camera it was rendered with" % call)
        for name, cam in (("cur", cur), ("prev", prev if hist_in is not None else None)):
            if cam is not None and not (isinstance(cam, (tuple, list)) and len(cam) == 2):
                raise ArtError("%s: %s: a camera is (cam_pos, cam_matrix)" % (call, name))
        if cur is None:
            raise ArtError("%s: cur: a camera is (cam_pos, cam_matrix)" % call)
        dev = lo_color.device
        _check_devices(planes, dev)
        if int(n_colours) < 1:
            raise ArtError("%s: n_colours must be at least 1, not %s" % (call, n_colours))
        p = params_struct()()
        p.t.cur = self.temporal_camera(cur, w, h)
        if hist_in is not None:
            p.t.prev = self.temporal_camera(prev, int(hist_in.shape[2]), int(hist_in.shape[1]))
        p.t.n_colours, p.t.max_history = int(n_colours), int(TEMPORAL_MAX_HISTORY if max_history is None else max_history)
        p.t.scale = float(scale)
        p.t.depth_tol = float(TEMPORAL_DEPTH_TOL if depth_tol is None else depth_tol)
        p.t.normal_min = float(TEMPORAL_NORMAL_MIN if normal_min is None else normal_min)
        p.lo_width, p.lo_height = lw, lh
        p.jitter[0], p.jitter[1] = float(jitter[0]), float(jitter[1])
        bound = min(float(np.float32(w) / np.float32(lw)), float(np.float32(h) / np.float32(lh)))
        p.radius = min(TEMPORAL_UPSAMPLE_RADIUS, bound) if radius is None else float(radius)
        p.min_confidence = float(min_confidence)
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        var = torch.empty((h, w), dtype=torch.float32, device=dev)
        length = torch.empty((h, w), dtype=torch.float32, device=dev)
        new = torch.empty((3, h, w, 4), dtype=torch.float32, device=dev)
        fallback = torch.empty((h, w), dtype=torch.uint8, device=dev) if want_fallback else None
        c_lo = ArtTemporalUpsampleGuides(*[_ptr(gl[k]) for k in GUIDES], None)
        c_hi = ArtTemporalUpsampleGuides(*[_ptr(gh[k]) for k in GUIDES], _ptr(motion))
        _check(self.lib.art_temporal_upsample_device(C.byref(p), lo_color.data_ptr(), lo_moments.data_ptr(), C.byref(c_lo), C.byref(c_hi), _ptr(hist_in),
                                                     new.data_ptr(), out.data_ptr(), var.data_ptr(), length.data_ptr(), _ptr(fallback),
                                                     _handle(_stream(torch, dev))))
        return (out, var, length, new, fallback) if want_fallback else (out, var, length, new)
