"""The display transform (art_auto_exposure_device, art_display_device; include/art_hip.h states the arithmetic): the parameter structs
and constants of the C entries and the torch-facing methods, which Backend inherits.  The package's one tensor check, its device check and
its error type are the package's own: they are looked up when a method runs, so this module imports nothing of the package while the
package is being imported."""
import ctypes as C
import sys

LAYOUT_ADA_XY, LAYOUT_ROW_MAJOR = 0, 1      # include/art_hip.h, as in the package


class ArtExposureParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("scale", C.c_float), ("min_log2", C.c_float), ("max_log2", C.c_float),
                ("low_fraction", C.c_float), ("high_fraction", C.c_float), ("key", C.c_float), ("adapt", C.c_float),
                ("min_exposure", C.c_float), ("max_exposure", C.c_float)]


class ArtDisplayParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("scale", C.c_float), ("exposure", C.c_float), ("curve", C.c_int32),
                ("transfer", C.c_int32), ("white", C.c_float), ("dither", C.c_int32), ("layout", C.c_int32)]


CURVE_REFERENCE, CURVE_LINEAR, CURVE_REINHARD, CURVE_ACES = 0, 1, 2, 3
TRANSFER_SQRT, TRANSFER_SRGB, TRANSFER_GAMMA22 = 0, 1, 2
STATE_WORDS = 4 + 256       # exposure, mean_log2, counted, frames, then the histogram (include/art_hip.h)


class DisplayCalls:
    """What Backend gains: exposure_state, auto_exposure_torch, display_torch (self.lib is the loaded library)."""

    def exposure_state(self, device="cuda"):
        """A fresh state for auto_exposure_torch: art_exposure_state_bytes() of zeroed device memory as an int32 tensor (the words of
        include/art_hip.h: exposure and mean_log2 as float bits, counted, frames, then the 256 bins)."""
        torch = sys.modules.get("torch") or __import__("torch")
        return torch.zeros(int(self.lib.art_exposure_state_bytes()) // 4, dtype=torch.int32, device=device)

    def auto_exposure_torch(self, color, state, scale=1.0, min_log2=-12.0, max_log2=4.0, low_fraction=0.5, high_fraction=0.95, key=0.18,
                            adapt=1.0, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10):
        """Auto-exposure from the histogram of log2 luminance (art_auto_exposure_device; include/art_hip.h states the arithmetic).
        color: float32 [H, W, 3] (the tensor of bind_accum viewed so is accepted as it is, scale = 1 / spp); state: the tensor of
        exposure_state(), updated in place: its first word is the exposure display_torch(state=...) reads on the device.  Returns
        state, enqueued on torch.cuda.current_stream() without waiting for it.  Every tensor is checked before any C call."""
        from . import _Plane, _check, _check_devices, _check_planes, _colour_frame, _handle, _image_plane, _stream
        torch = sys.modules.get("torch")
        call = "auto_exposure_torch"
        h, w = _colour_frame(torch, call, color)
        planes = [_image_plane(call, h, w, "color", color, 3), _Plane(call + ": state", state, "int32", (STATE_WORDS,))]
        _check_planes(torch, planes)
        _check_devices(planes, color.device)
        p = ArtExposureParams(w, h, float(scale), float(min_log2), float(max_log2), float(low_fraction), float(high_fraction), float(key),
                              float(adapt), float(min_exposure), float(max_exposure))
        _check(self.lib.art_auto_exposure_device(C.byref(p), color.data_ptr(), state.data_ptr(), _handle(_stream(torch, color.device))))
        return state

    def display_torch(self, color, state=None, exposure=1.0, curve=CURVE_ACES, transfer=TRANSFER_SRGB, dither=True, layout=LAYOUT_ROW_MAJOR,
                      out=None, want_ldr=False, scale=1.0, white=4.0, want_screen=True):
        """The HDR plane as screen pixels (art_display_device; include/art_hip.h states the arithmetic): exposure, tone curve, transfer
        function, 8 bits per channel.  color: float32 [H, W, 3]; state: the tensor of auto_exposure_torch, whose exposure is read on
        the device, or None for `exposure`.  curve = CURVE_REFERENCE gives the words download() would make of the plane (scale =
        1 / spp), and has no ldr plane.  Returns the screen words r | g << 8 | b << 16 as an int32 tensor, [H, W] (what save_bmp takes
        after .cpu().numpy()) or [W, H] with LAYOUT_ADA_XY; out: that tensor, or None for a new one.  want_ldr: returns (screen, ldr)
        with ldr the float32 [H, W, 3] (or [W, H, 3]) values after the transfer, before quantisation; want_screen=False: screen is None.
        Enqueued on torch.cuda.current_stream() without waiting for it.  Every tensor is checked before any C call."""
        from . import ArtError, _Plane, _check, _check_devices, _check_planes, _colour_frame, _handle, _image_plane, _ptr, _stream
        torch = sys.modules.get("torch")
        call = "display_torch"
        h, w = _colour_frame(torch, call, color)
        shape = (h, w) if layout == LAYOUT_ROW_MAJOR else (w, h)
        planes = [_image_plane(call, h, w, "color", color, 3), _Plane(call + ": state", state, "int32", (STATE_WORDS,), True),
                  _Plane(call + ": out", out, "int32", shape, True)]
        _check_planes(torch, planes)
        _check_devices(planes, color.device)
        if not want_screen and not want_ldr:
            raise ArtError("display_torch: neither the screen nor the ldr plane is wanted")
        if not want_screen and out is not None:
            raise ArtError("display_torch: out is the screen plane, which want_screen=False leaves out")
        if want_screen and out is None:
            out = torch.empty(shape, dtype=torch.int32, device=color.device)
        ldr = torch.empty(shape + (3,), dtype=torch.float32, device=color.device) if want_ldr else None
        p = ArtDisplayParams(w, h, float(scale), float(exposure), int(curve), int(transfer), float(white), 1 if dither else 0, int(layout))
        _check(self.lib.art_display_device(C.byref(p), color.data_ptr(), _ptr(state), _ptr(out), _ptr(ldr), _handle(_stream(torch, color.device))))
        return (out, ldr) if want_ldr else out
