"""The refusal cases of art_bloom_device (tests/golden/bloom_refusals.json, whose "about" states the format) and the one routine that
makes a case's call: tests/test_bloom_abi.py runs the cases that need no device over pointers that are never dereferenced,
tests/test_gpu_bloom.py runs all of them over device planes.  Unlike art_firefly_device's, this call's overlap refusals need no
device: they come with the parameter checks."""
import ctypes as C
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "art_bloom_device"
PLANES = ("color3f", "exposure_state", "out3f", "bloom3f")
PER_PIXEL = {"color3f": 12, "out3f": 12, "bloom3f": 12}
STATE_BYTES = 1040
OUTPUTS = ("out3f", "bloom3f")


def load():
    with open(os.path.join(HERE, "golden", "bloom_refusals.json")) as f:
        rec = json.load(f)
    return tuple(rec["frame"]), rec["cases"]


def plane_bytes(frame):
    """bytes of every plane of the good call"""
    W, H = frame
    return dict({k: v * W * H for k, v in PER_PIXEL.items()}, exposure_state=STATE_BYTES)


def _number(v):
    return float(v) if isinstance(v, str) else v


def call(art, L, frame, case, base, host=None, short=None):
    """(rc, art_last_error() text) of one case.  base: {plane: address} of the good call's planes; host: an address in host memory;
    short(bytes) -> the address of device memory of that size"""
    W, H = frame
    v = dict(width=W, height=H, levels=6, karis=1, variant=0, scale=1.0, exposure=1.0, threshold=1.0, knee=0.5, scatter=0.7, strength=0.05)
    v.update({k: _number(x) for k, x in case.get("set", {}).items()})
    p = art.bloom.ArtBloomParams(*[v[n] for n, _ in art.bloom.ArtBloomParams._fields_])
    sizes = plane_bytes(frame)
    ptr = {k: base[k] for k in PLANES}
    null_p = False
    for key, how in case.get("args", {}).items():
        if how == "null":
            if key == "p":
                null_p = True
            else:
                ptr[key] = None
        elif how == "host":
            ptr[key] = host
        elif how == "short":
            ptr[key] = short(sizes[key] - PER_PIXEL.get(key, 4))
        elif how.startswith("over "):
            ptr[key] = base[how[5:]] + 16
        elif how.startswith("is "):
            ptr[key] = base[how[3:]]
        else:
            raise ValueError(how)
    rc = getattr(L, NAME)(None if null_p else C.byref(p), *[ptr[k] for k in PLANES], None)
    return rc, (L.art_last_error().decode() if rc else "")


def check(art, L, frame, case, base, **kw):
    rc, text = call(art, L, frame, case, base, **kw)
    assert rc != 0 and text.startswith(NAME + ": ") or (rc != 0 and case["needs_device"]), (case["name"], rc, text)
    assert case["message"] in text, (case["name"], text)
