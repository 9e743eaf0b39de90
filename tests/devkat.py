"""ctypes binding of tests/device_kat/libdevice_kat.so (TEST-ONLY: the product's ART_HD functions as a gfx950 code object of their own,
one known-answer op per launch) and of the same ops in the host build (tests/host_sim, hs_kat_run).  The op table mirrors
tests/device_kat/kat_ops.h: name -> (op number, words in, words out, parameter bytes)."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostsim

HERE = os.path.dirname(os.path.abspath(__file__))
LIGHT_BYTES, MATERIAL_BYTES = 76, 40           # sizeof(DevLight), sizeof(DevMaterial) = the ABI's ArtLight / ArtMaterial
CAMERA_BYTES = 80                              # sizeof(kat::CameraParams): width, height, aa_on, cam_z, cam_matrix[16]

OPS = {name: (k,) + shape for k, (name, shape) in enumerate([
    ("sincos", (1, 2, 0)), ("tan", (1, 2, 0)), ("apow", (2, 1, 0)), ("sqrt", (1, 1, 0)), ("rcp", (1, 1, 0)), ("div", (2, 1, 0)),
    ("normalize", (3, 3, 0)), ("reflect", (6, 3, 0)), ("perpendicular", (3, 3, 0)), ("log_pos", (1, 2, 0)), ("exp_small", (1, 2, 0)),
    ("sample_cosine", (9, 3, 0)), ("sample_cosine_fixed", (9, 3, 0)), ("fresnel", (3, 1, 0)),
    ("light_sample", (5, 10, LIGHT_BYTES)), ("light_eval_pdf", (7, 1, LIGHT_BYTES)), ("sphere_light_pdf", (3, 1, LIGHT_BYTES)),
    ("pdf_area_to_solid", (3, 1, 0)), ("bsdf_sample", (8, 8, MATERIAL_BYTES)), ("bsdf_eval", (9, 4, MATERIAL_BYTES)),
    ("tri_raw", (15, 4, 0)), ("sphere", (10, 2, 0)), ("cornell", (6, 5, 24)), ("quad", (6, 2, LIGHT_BYTES)), ("slab", (13, 8, 0)),
    ("cand_wins", (4, 1, 0)), ("sincos_f64", (1, 4, 0)),
    ("camera_dir", (2, 3, CAMERA_BYTES)), ("resolve", (4, 1, 0)), ("round_u32", (1, 1, 0)), ("colour_lum", (3, 1, 0))])}

_dev = None
_sig = [C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]


def device_lib():
    global _dev
    if _dev is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "device_kat")])
        L = C.CDLL(os.path.join(HERE, "device_kat", "libdevice_kat.so"))
        L.dk_run.argtypes = _sig; L.dk_run.restype = C.c_int
        L.dk_last_error.restype = C.c_char_p
        _dev = L
    return _dev


def _call(fn, err, op, inp, params):
    k, nin, nout, pbytes = OPS[op]
    inp = np.ascontiguousarray(inp, np.uint32).reshape(-1, nin)          # words: the bits travel as they are
    par = np.frombuffer(bytes(params) if params is not None else b"", np.uint8).copy()
    assert par.size >= pbytes, (op, par.size, pbytes)
    out = np.zeros((inp.shape[0], nout), np.uint32)
    rc = fn(k, inp.shape[0], inp.ctypes.data, nin, out.ctypes.data, nout, par.ctypes.data if par.size else None, int(par.size))
    if rc:
        raise RuntimeError("%s: %d %s" % (op, rc, err().decode()))
    return out


def run_device(op, inp, params=None):
    """op on the GPU over the items of inp (n x words-in, uint32 words) -> n x words-out uint32 words"""
    L = device_lib()
    return _call(L.dk_run, L.dk_last_error, op, inp, params)


def run_host(art, op, inp, params=None):
    """the same op through the g++ build of the same per-item text"""
    L = hostsim.lib(art)
    L.hs_kat_run.argtypes = _sig; L.hs_kat_run.restype = C.c_int
    return _call(L.hs_kat_run, L.hs_last_error, op, inp, params)


def same_words(a, b):
    """the comparison rule of the known-answer tests: both NaN (payload and sign free), or the same bits.  Returns the mask of items that
    differ.  Words that are not floats (hit keys, halves of a binary64) never look like a NaN pair unless both do, and then a differing
    payload would be missed -- the callers compare such columns with bits_differ."""
    fa, fb = a.view(np.float32), b.view(np.float32)
    ok = (a == b) | (np.isnan(fa) & np.isnan(fb))
    return ~ok.all(axis=1)


def bits_differ(a, b):
    return ~(a == b).all(axis=1)
