"""The refusal cases of art_temporal_upsample_device (tests/golden/temporal_upsample_refusals.json, whose "about" states the format) and
the one routine that makes a case's call: tests/test_temporal_upsample_abi.py runs the cases that need no device over pointers that are
never dereferenced, tests/test_gpu_temporal_upsample.py runs all of them over device planes."""
import ctypes as C
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "art_temporal_upsample_device"
PLANES = ("lo_color3f", "lo_moments2f", "lo.normal3f", "lo.depth", "lo.id", "hi.normal3f", "hi.depth", "hi.id", "hi.motion3f", "hist_in", "hist_out", "out3f",
          "variance_out", "length_out", "fallback1b")
IDENT = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]


def load():
    with open(os.path.join(HERE, "golden", "temporal_upsample_refusals.json")) as f:
        rec = json.load(f)
    return tuple(rec["frame"]), rec["cases"]


def plane_bytes(frame):
    """bytes of every plane of the good call"""
    W, H, LW, LH = frame
    n, nl = W * H, LW * LH
    return {"lo_color3f": 12 * nl, "lo_moments2f": 8 * nl, "lo.normal3f": 12 * nl, "lo.depth": 4 * nl, "lo.id": 4 * nl, "hi.normal3f": 12 * n, "hi.depth": 4 * n,
            "hi.id": 4 * n, "hi.motion3f": 12 * n, "hist_in": 48 * n, "hist_out": 48 * n, "out3f": 12 * n, "variance_out": 4 * n, "length_out": 4 * n, "fallback1b": n}


def _number(v):
    return float(v) if isinstance(v, str) else v


def call(art, L, frame, case, base, host=None, short=None):
    """(rc, art_last_error() text) of one case.  base: {plane: address} of the good call's planes (hi.motion3f and lo.motion3f are not
    part of the good call: base holds an address for 'given' and 'host' to use); host: an address in host memory; short(bytes) -> the
    address of device memory of that size"""
    W, H, LW, LH = frame
    TU = art.temporal_upsample
    p = TU.params_struct()()
    for cam in (p.t.cur, p.t.prev):
        for k in range(16):
            cam.cam_matrix[k] = IDENT[k]
        cam.width, cam.height = W, H
    p.t.n_colours, p.t.max_history, p.t.scale, p.t.depth_tol, p.t.normal_min = 1, 16, 1.0, 0.05, 0.9
    p.lo_width, p.lo_height, p.radius, p.min_confidence = LW, LH, 1.0, 0.25
    for key, v in case.get("set", {}).items():
        v = _number(v)
        if key.startswith(("cur.", "prev.")):
            cam = p.t.cur if key.startswith("cur.") else p.t.prev
            field = key.split(".")[1]
            if field[0] == "m" and field[1:].isdigit():
                cam.cam_matrix[int(field[1:])] = v
            else:
                setattr(cam, field, v)
        elif key in ("jitter0", "jitter1"):
            p.jitter[int(key[-1])] = v
        elif key in ("lo_width", "lo_height", "radius", "min_confidence"):
            setattr(p, key, v)
        else:
            setattr(p.t, key, v)
    sizes = plane_bytes(frame)
    one_pixel = {k: sizes[k] // (LW * LH if k.startswith("lo") else W * H) for k in sizes}
    ptr = {k: base[k] for k in PLANES if k != "hi.motion3f"}
    ptr["hi.motion3f"] = ptr["lo.motion3f"] = None
    null = set()
    for key, how in case.get("args", {}).items():
        if how == "null":
            null.add(key) if key in ("p", "lo", "hi") else ptr.__setitem__(key, None)
        elif how == "given":
            ptr[key] = base["hi.motion3f"]
        elif how == "host":
            ptr[key] = host
        elif how == "short":
            ptr[key] = short(sizes[key] - one_pixel[key])
        elif how.startswith("over "):
            ptr[key] = base[how[5:].replace(" ", ".")] + 16
        else:
            raise ValueError(how)
    lo = TU.ArtTemporalUpsampleGuides(ptr["lo.normal3f"], ptr["lo.depth"], ptr["lo.id"], ptr["lo.motion3f"])
    hi = TU.ArtTemporalUpsampleGuides(ptr["hi.normal3f"], ptr["hi.depth"], ptr["hi.id"], ptr["hi.motion3f"])
    rc = getattr(L, NAME)(None if "p" in null else C.byref(p), ptr["lo_color3f"], ptr["lo_moments2f"], None if "lo" in null else C.byref(lo),
                          None if "hi" in null else C.byref(hi), ptr["hist_in"], ptr["hist_out"], ptr["out3f"], ptr["variance_out"], ptr["length_out"],
                          ptr["fallback1b"], None)
    return rc, (L.art_last_error().decode() if rc else "")


def check(art, L, frame, case, base, **kw):
    rc, text = call(art, L, frame, case, base, **kw)
    assert rc != 0 and text.startswith(NAME + ": ") or (rc != 0 and case["needs_device"]), (case["name"], rc, text)
    assert case["message"] in text, (case["name"], text)
