"""numpy reference of art_radiance_rays_device's two ends, written from the comment in include/art_hip.h (TEST INFRASTRUCTURE ONLY):
how a ray's path values go into the caller's planes, and what a ray's path starts from.  binary32 throughout: every operation is one
numpy float32 operation, so nothing is contracted."""
import numpy as np

F = np.float32
FLAG_ALIVE, FLAG_PREV_SPEC = 1, 2
KEY_MISS = 0x7FFFFFFF
FLOAT_LAST = F(3.4028234663852886e38)
# art_scene.h HotField: the words of a bank's block, field f of item w at word f * stride + w (HF_HIT: 4 words per item)
HF_OX, HF_OY, HF_OZ, HF_DX, HF_DY, HF_DZ, HF_HIT, HF_SHT, HF_PDF, HF_FLAGS, HF_SHMIN, HF_SLOT, HOT_FIELDS = 0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15


def luminance(c):
    """l = (0.2126f r + 0.7152f g) + 0.0722f b"""
    c = np.asarray(c, F)
    return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]).astype(F)


def accumulate(values, radiance=None, moments=None):
    """values [n, samples, 3]: path k of ray i.  For k = 0 .. samples - 1 in that order: out = s_k + out per channel; S1 = l + S1;
    S2 = l * l + S2.  radiance [n, 3] / moments [n, 2]: what the planes held before (None: zeros).  Returns new (radiance, moments)."""
    values = np.asarray(values, F)
    n = values.shape[0]
    out = np.zeros((n, 3), F) if radiance is None else np.array(radiance, F)
    mom = np.zeros((n, 2), F) if moments is None else np.array(moments, F)
    with np.errstate(all="ignore"):
        for k in range(values.shape[1]):
            s = values[:, k]
            out = (s + out).astype(F)
            l = luminance(s)
            mom[:, 0] = (l + mom[:, 0]).astype(F)
            mom[:, 1] = ((l * l).astype(F) + mom[:, 1]).astype(F)
    return out, mom


def raygen_words(origins, dirs, samples):
    """The hot words raygen leaves for the n * samples slots of a batch (slot = sample * n + ray), as {field: uint32 [P]} (HF_HIT: [P, 4],
    for a scene without analytic primitives: the unbounded miss).  A path starts as a camera sample does: previous pdf 1, alive, previous
    bounce specular; the direction as given."""
    o = np.ascontiguousarray(origins, F); d = np.ascontiguousarray(dirs, F)
    n = o.shape[0]
    P = n * samples
    ray = np.arange(P) % n
    u = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    w = {HF_OX: u(o[ray, 0]), HF_OY: u(o[ray, 1]), HF_OZ: u(o[ray, 2]), HF_DX: u(d[ray, 0]), HF_DY: u(d[ray, 1]), HF_DZ: u(d[ray, 2]),
         HF_PDF: u(np.full(P, 1.0, F)), HF_FLAGS: np.full(P, FLAG_ALIVE | FLAG_PREV_SPEC, np.uint32), HF_SLOT: np.arange(P, dtype=np.uint32),
         HF_SHT: u(np.full(P, -1.0, F)), HF_SHMIN: u(np.zeros(P, F))}
    hit = np.zeros((P, 4), np.uint32)
    hit[:, 0] = np.array([FLOAT_LAST], F).view(np.uint32)[0]
    hit[:, 1] = KEY_MISS
    w[HF_HIT] = hit
    return w
