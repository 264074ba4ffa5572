"""float64 numpy model of points2surf_amd.normals: the kNN neighbourhood with the id tie-break, the
covariance and its eigenvectors through ``eigh``, and the orientation as Kruskal's algorithm in the total order
(w, min id, max id) with a parity union-find.  The minimum spanning forest under a total order is unique, so the signs the
device's Boruvka rounds give must equal these bit for bit.

Also the clouds with analytic normals that both the CPU and the GPU tests use.
"""
import numpy as np


def knn(points, k, chunk=512):
    """ids [n, k] int32 of the k nearest points of every point (itself included): float64 d2 = (dx dx + dy dy) + dz dz from
    the float32 coordinates, ascending, ties by id -- what p2s_knn_patch returns"""
    p = np.asarray(points, np.float32).astype(np.float64)
    n = p.shape[0]
    out = np.empty((n, k), np.int32)
    for a in range(0, n, chunk):
        d = p[a:a + chunk, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[a:a + chunk] = np.argsort(d2, axis=1, kind='stable')[:, :k]          # stable: equal distances stay in id order
    return out


def knn_tree(points, k, extra=4):
    """``knn`` for clouds too large for the brute force: the k + extra nearest of a cKDTree, re-ranked by the same float64
    distance and id.  Equal to ``knn`` unless more than ``extra`` points tie at the k-th distance"""
    from scipy.spatial import cKDTree
    p = np.asarray(points, np.float32).astype(np.float64)
    m = min(k + extra, p.shape[0])
    cand = np.sort(cKDTree(p).query(p, m)[1], axis=1)                            # by id, so that the stable sort keeps that order
    d = p[:, None, :] - p[cand]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.take_along_axis(cand, np.argsort(d2, axis=1, kind='stable'), axis=1)[:, :k].astype(np.int32)


def covariance(points, ids):
    """C [n, 3, 3] float64 = sum over the neighbourhood of (p - c)(p - c)^T, c its centroid"""
    p = np.asarray(points, np.float32).astype(np.float64)[ids]                   # [n, k, 3]
    q = p - p.mean(axis=1, keepdims=True)
    return np.einsum('nki,nkj->nij', q, q)


def estimate(points, k, ids=None):
    """(normals [n, 3] float64 unit, or 0 where C = 0; variation [n] float64; C; eigenvalues [n, 3] ascending; ids)"""
    ids = knn(points, k) if ids is None else ids
    C = covariance(points, ids)
    lam, vec = np.linalg.eigh(C)
    nrm = vec[:, :, 0].copy()
    tr = lam.sum(axis=1)
    zero = ~(np.abs(C).max(axis=(1, 2)) > 0.0)
    var = np.divide(np.maximum(lam[:, 0], 0.0), tr, out=np.zeros_like(tr), where=tr > 0.0)
    nrm[zero] = 0.0
    var[zero] = 0.0
    return nrm, var, C, lam, ids


def edges(ids):
    """the undirected edges {i, j}, i != j, j among the k nearest of i or the reverse: (lo [E], hi [E]), unique"""
    n, k = ids.shape
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = ids.reshape(-1).astype(np.int64)
    keep = i != j
    lo, hi = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    pair = np.unique(lo * n + hi)
    return pair // n, pair % n


def orient(points, normals, k=None, ids=None):
    """(normals float32 with consistent signs, component [n] int32, info): ``normals`` float32 [n, 3]; only signs change.
    info: components, edges, flipped"""
    pts = np.asarray(points, np.float32)
    nrm = np.ascontiguousarray(normals, np.float32)
    n = pts.shape[0]
    ids = knn(pts, k) if ids is None else ids
    lo, hi = edges(ids)
    a, b = nrm[lo].astype(np.float64), nrm[hi].astype(np.float64)
    d = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    w = 1.0 - np.abs(d)
    order = np.lexsort((hi, lo, w))
    parent = list(range(n))
    par = [0] * n                                    # parity of a node against its parent

    def find(x):
        path, acc = [], 0
        while parent[x] != x:
            path.append(x)
            x = parent[x]
        # compress: the parity of every node on the path against the root
        for y in reversed(path):
            acc ^= par[y]
            par[y] = acc
            parent[y] = x
        return x

    for e in order:
        i, j = int(lo[e]), int(hi[e])
        ri, rj = find(i), find(j)
        if ri == rj:
            continue
        flip = 1 if d[e] < 0.0 else 0
        parent[rj] = ri
        par[rj] = par[i] ^ par[j] ^ flip
    root = np.empty(n, np.int64)
    sign = np.empty(n, np.int64)
    for i in range(n):
        root[i] = find(i)
        sign[i] = par[i] if parent[i] != i else 0
    z = pts[:, 2] + np.float32(0.0)
    component = np.empty(n, np.int32)
    flip = np.zeros(n, bool)
    roots = np.unique(root)
    for r in roots:
        m = np.nonzero(root == r)[0]
        seed = m[np.argmax(z[m])]                    # the first of equal ones: the smallest id
        nz = -nrm[seed, 2] if sign[seed] else nrm[seed, 2]
        g = 1 if nz < 0 else 0
        flip[m] = (sign[m] ^ g).astype(bool)
        component[m] = m.min()
    out = nrm.copy()
    out[flip] = -out[flip]
    return out, component, dict(components=int(roots.size), edges=int(lo.size), flipped=int(flip.sum()))


# ---- clouds with analytic outward normals -------------------------------------------------------------------------------

def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def sphere(n=3000, radius=0.4, centre=(0.0, 0.0, 0.0), sigma=0.0, seed=0):
    """(points float32 [n, 3], outward normals float64)"""
    rng = np.random.default_rng(seed)
    u = _unit(rng, n)
    p = np.asarray(centre) + radius * u
    if sigma > 0.0:
        p = p + sigma * rng.standard_normal((n, 3))
    return p.astype(np.float32), u


def torus(n=4000, R=0.3, r=0.12, seed=0):
    rng = np.random.default_rng(seed)
    # uniform by area: the density along the tube's angle is proportional to R + r cos(v)
    v = np.empty(0)
    while v.size < n:
        cand = rng.uniform(0.0, 2.0 * np.pi, 2 * n)
        v = np.concatenate([v, cand[rng.uniform(0.0, R + r, 2 * n) < R + r * np.cos(cand)]])
    v = v[:n]
    u = rng.uniform(0.0, 2.0 * np.pi, n)
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=1)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    return p.astype(np.float32), nrm


def two_spheres(seed=0):
    pa, na = sphere(2000, 0.2, (-0.25, 0.0, 0.0), seed=seed)
    pb, nb = sphere(1500, 0.15, (0.3, 0.0, 0.1), seed=seed + 1)
    return np.concatenate([pa, pb]), np.concatenate([na, nb])


def noisy_sphere(seed=0):
    return sphere(3000, 0.4, sigma=0.004, seed=seed)


def oriented(points, k, tree=False):
    """the model end to end: float32 normals (eigh, rounded) oriented; (normals, component, info, variation)"""
    nrm, var, _, _, ids = estimate(points, k, knn_tree(points, k) if tree else None)
    out, comp, info = orient(points, nrm.astype(np.float32), ids=ids)
    return out, comp, info, var
