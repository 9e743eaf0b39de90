"""Numbering-independent fingerprint of an exported wide tree (the one tests/test_gpu_lbvh.py compares the host and the GPU SAH builder
with), for tests that compare trees whose nodes may be numbered differently."""
import numpy as np


def tree_signature(nodes, tris, info):
    """Numbering-independent fingerprint of a wide tree: bottom-up, a node's hash mixes, in slot order, every child's box (bit
    patterns) with the prim ids of a leaf or the hash of an inner child.  Two trees get the same root hash iff they hold the same
    boxes, the same leaves and the same slot order everywhere (up to hash collisions)."""
    W = info.node_width
    nodes = np.asarray(nodes, np.float32).reshape(-1, 8 * W); tris = np.asarray(tris, np.float32).reshape(-1, 12)
    N = nodes.shape[0]
    prim = tris[:, 9].view(np.int32).astype(np.uint64)
    ref = nodes[:, 3:4 * W:4].view(np.int32); cnt = nodes[:, 4 * W + 3:8 * W:4].view(np.int32)
    box = np.concatenate([nodes[:, :4 * W].reshape(N, W, 4)[:, :, :3], nodes[:, 4 * W:].reshape(N, W, 4)[:, :, :3]], axis=2).view(np.uint32).astype(np.uint64)
    used = ref >= 0; inner = used & (cnt == 0); leaf = used & (cnt > 0)
    M = np.uint64(0x9E3779B97F4A7C15)

    def mix(h, v):
        h = (h ^ v) * M
        return h ^ (h >> np.uint64(29))

    order = [np.array([0])]
    while True:
        f = order[-1]
        kids = ref[f][inner[f]]
        if kids.size == 0:
            break
        order.append(kids)
    H = np.zeros(N, np.uint64)
    with np.errstate(over="ignore"):
        for lvl in reversed(order):
            h = np.full(lvl.size, 1469598103934665603, np.uint64)
            for j in range(W):
                u = used[lvl, j]
                hj = np.full(lvl.size, 7, np.uint64)
                for a in range(6):
                    hj = mix(hj, box[lvl, j, a])
                lf = leaf[lvl, j]; inn = inner[lvl, j]
                for k in range(W):
                    m = lf & (cnt[lvl, j] > k)
                    pk = np.zeros(lvl.size, np.uint64)
                    pk[m] = prim[(ref[lvl, j][m] + k)] + np.uint64(1)
                    hj = mix(hj, pk)
                ch = np.zeros(lvl.size, np.uint64)
                ch[inn] = H[ref[lvl, j][inn]]
                hj = mix(hj, ch)
                h = np.where(u, mix(h, hj), mix(h, np.uint64(3)))
            H[lvl] = h
    return int(H[0]), N, int(leaf.sum())
