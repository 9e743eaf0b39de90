"""art_aovs_rays_device in numpy, written from the contract in include/art_hip.h (not from the kernels): the eight planes from the ArtHit
words of the rays, the rays themselves, the group size, the background and the albedo table.  Every operation is one binary32 operation
of numpy (no fused multiply-add, no wider intermediate): the sums are a left fold, the mean one division by (float)K."""
import numpy as np

F = np.float32
PLANES = ("albedo", "normal", "position", "depth", "alpha", "prim_type", "prim_index", "mat")


def group_mean(v, k):
    """v[G, k, ...] float32 -> [G, ...]: (((v_0 + v_1) + ...) + v_{k-1}) / (float)k"""
    v = np.asarray(v, F)
    assert v.shape[1] == k
    acc = v[:, 0]
    with np.errstate(all="ignore"):
        for s in range(1, k):
            acc = (acc + v[:, s]).astype(F)
        return (acc / F(k)).astype(F)


def position(o, d, t):
    """o + t * d per component: one multiply, then one add"""
    with np.errstate(all="ignore"):
        td = (np.asarray(t, F)[..., None] * np.asarray(d, F)).astype(F)
        return (np.asarray(o, F) + td).astype(F)


def aov_rays_ref(raw, origins, dirs, group, background, table):
    """raw: [n, 11] int32, the ArtHit words trace_rays_torch returns for the rays (with the same tnear / tfar); origins, dirs: [n, 3]
    float32 as the caller gave them; table: [n_materials, 3] float32, the albedo of every material.  Returns the dict of the eight
    planes, one element per group of `group` consecutive rays."""
    raw = np.ascontiguousarray(raw, np.int32).reshape(-1, 11)
    n, k = raw.shape[0], int(group)
    assert n % k == 0
    g = n // k
    f = raw.view(F)
    hit = raw[:, 1] == 1
    mat = raw[:, 5]
    alb = np.where(hit[:, None], np.asarray(table, F)[np.where(hit, mat, 0)], np.asarray(background, F)).astype(F)
    nrm = np.where(hit[:, None], f[:, 6:9], F(0.0)).astype(F)
    pos = np.where(hit[:, None], position(origins, dirs, f[:, 0]), F(0.0)).astype(F)
    dep = np.where(hit, f[:, 0], F(0.0)).astype(F)
    cov = hit.astype(F)
    first = raw.reshape(g, k, 11)[:, 0]
    return dict(albedo=group_mean(alb.reshape(g, k, 3), k), normal=group_mean(nrm.reshape(g, k, 3), k), position=group_mean(pos.reshape(g, k, 3), k),
                depth=group_mean(dep.reshape(g, k), k), alpha=group_mean(cov.reshape(g, k), k),
                prim_type=first[:, 2].copy(), prim_index=first[:, 3].copy(), mat=first[:, 5].copy())
