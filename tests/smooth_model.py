"""The numpy model of DESIGN 4.8 f17 (include/p2s_hip.h: p2s_mesh_smooth, rules b to e), with no device: the same neighbours,
classes, half-steps and report, in the same float64 operations in the same order, so that the device is compared with it for
EQUALITY of bytes.  The rows are padded to the largest degree of their bucket and added column by column under a mask: the
sequential order of rule d.  Also the meshes of the tests: tetrahedron, octahedron, icosphere, open grid, cone, strips and the
hand-made class cases."""
import numpy as np

EINVAL = -1
FREE, CURVE, BOUNDARY_FIXED, NONMANIFOLD, MASKED, UNREFERENCED = 0, 1, 2, 3, 4, 5
MODES = {'fixed': 0, 'curve': 1, 'free': 2}
SHORT = 32                                          # rows of up to this many neighbours share one padded block


def edges(faces):
    """the undirected edges of the face list -> a [E], b [E] (a < b, ascending in (a, b)), and the faces on each"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        z = np.zeros(0, np.int64)
        return z, z, z
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key, cnt = np.unique((e.min(axis=1) << 32) | e.max(axis=1), return_counts=True)
    return key >> 32, key & 0xffffffff, cnt.astype(np.int64)


def classes(V, a, b, cnt, mode, fixed=None):
    """rule c -> the class byte of every vertex"""
    deg = np.bincount(a, minlength=V) + np.bincount(b, minlength=V)
    one = cnt == 1
    bdeg = np.bincount(a[one], minlength=V) + np.bincount(b[one], minlength=V)
    many = cnt > 2
    nm = (np.bincount(a[many], minlength=V) + np.bincount(b[many], minlength=V)) > 0
    cls = np.zeros(V, np.uint8)
    if mode != 2:
        cls[(bdeg > 0) & (bdeg == 2)] = CURVE if mode == 1 else BOUNDARY_FIXED
        cls[(bdeg > 0) & (bdeg != 2)] = BOUNDARY_FIXED
        cls[nm] = NONMANIFOLD
    cls[deg == 0] = UNREFERENCED
    if fixed is not None:
        cls[np.asarray(fixed).reshape(-1) != 0] = MASKED
    return cls


def rows(V, a, b, cnt, cls):
    """rule b and c -> start [V + 1], col [start[V]]: the neighbours that a vertex of class 0 or 1 reads, ascending"""
    i, j, one = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([cnt, cnt]) == 1
    keep = (cls[i] == FREE) | ((cls[i] == CURVE) & one)
    key = np.sort((i[keep] << 32) | j[keep])
    start = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(key >> 32, minlength=V), out=start[1:])
    return start, key & 0xffffffff


def _blocks(start, col):
    """the moving vertices in two buckets (short and long rows): their ids, padded neighbour table and degrees"""
    d = np.diff(start)
    out = []
    for sel in ((d > 0) & (d <= SHORT), d > SHORT):
        ids = np.nonzero(sel)[0]
        if len(ids) == 0:
            continue
        dd = d[ids]
        k = np.arange(dd.max())
        mask = k[None, :] < dd[:, None]
        idx = np.where(mask, start[ids][:, None] + k[None, :], 0)
        out.append((ids, np.where(mask, col[idx], 0), mask, dd))
    return out


def half_step(P, blocks, w):
    """rule d on float32 positions P [V, 3] -> new float32 positions; the fixed vertices keep their bytes"""
    Q = P.copy()
    w = np.float64(w)
    with np.errstate(all='ignore'):
        for ids, nb, mask, dd in blocks:
            s = P[nb[:, 0]].astype(np.float64)
            for k in range(1, nb.shape[1]):
                s = np.where(mask[:, k, None], s + P[nb[:, k]].astype(np.float64), s)
            m = s / dd.astype(np.float64)[:, None]
            p = P[ids].astype(np.float64)
            Q[ids] = (p + w * (m - p)).astype(np.float32)
    return Q


def smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53, mode=0, fixed=None):
    """p2s_mesh_smooth: dict(rc, verts [V, 3] float32, cls [V] uint8, report [16] int64)"""
    P0 = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(P0)
    a, b, cnt = edges(f)
    cls = classes(V, a, b, cnt, mode, fixed)
    start, col = rows(V, a, b, cnt, cls)
    blocks = _blocks(start, col)
    steps = [lam] + ([mu] if mu != 0 else [])
    P, ran = P0, 0
    if len(col):
        for _ in range(iterations):
            for w in steps:
                P = half_step(P, blocks, w)
                ran += 1
    fin = np.isfinite(P)
    with np.errstate(all='ignore'):
        dd = P.astype(np.float64) - P0.astype(np.float64)
        dsq = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    ok = fin.all(axis=1)
    rep = np.zeros(16, np.int64)
    rep[0] = V | (len(f) << 32)
    rep[1:7] = np.bincount(cls, minlength=6)
    rep[7] = len(a)
    rep[8] = int(np.diff(start).max()) if V else 0
    rep[9] = ran
    rep[10] = np.array([dsq[ok].max() if ok.any() else 0.0], np.float64).view(np.int64)[0]
    rep[11] = int((~fin).sum())
    return dict(rc=EINVAL if rep[11] else 0, verts=P, cls=cls, report=rep)


def signed_volume(v, f):
    p = np.asarray(v, np.float64)[np.asarray(f, np.int64)]
    return float(np.einsum('ij,ij->i', p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- meshes
def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def icosphere(subdivisions, noise=0.0, seed=0):
    """a unit icosphere (12, 42, 162, 642, ... vertices), outward faces; Gaussian noise of sigma ``noise`` on every coordinate"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4],
         [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = g
    v = np.array(v, np.float64)
    if noise:
        v = v + np.random.default_rng(seed).normal(0.0, noise, v.shape)
    return v.astype(np.float32), np.array(f, np.int32)


def grid(nx, ny, noise=0.0, seed=0):
    """an open nx x ny grid of vertices in the plane z = 0 (spacing 1), two triangles per cell, noise on every coordinate"""
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing='xy')
    v = np.stack([x.ravel(), y.ravel(), np.zeros(nx * ny)], axis=1)
    if noise:
        v = v + np.random.default_rng(seed).normal(0.0, noise, v.shape)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx + 1], axis=1), np.stack([i, i + nx + 1, i + nx], axis=1)])
    return v.astype(np.float32), f.astype(np.int32)


def cone(n, seed=0):
    """a ring of n vertices closed by two apexes of n neighbours each: n + 2 vertices, 2 n faces, no boundary"""
    a = 2.0 * np.pi * np.arange(n) / n
    r = 1.0 + np.random.default_rng(seed).normal(0.0, 0.05, n)
    ring = np.stack([r * np.cos(a), r * np.sin(a), 0.1 * np.sin(7 * a)], axis=1)
    v = np.concatenate([ring, [[0.1, -0.2, 1.5], [0.05, 0.1, -0.7]]])
    i = np.arange(n)
    j = (i + 1) % n
    f = np.concatenate([np.stack([i, j, np.full(n, n)], axis=1), np.stack([j, i, np.full(n, n + 1)], axis=1)])
    return v.astype(np.float32), f.astype(np.int32)


def strip(n, seed=0):
    """n vertices in a zigzag strip of n - 2 triangles (none below 3 vertices)"""
    i = np.arange(n)
    v = np.stack([0.5 * i, (i % 2).astype(np.float64), np.zeros(n)], axis=1) + np.random.default_rng(seed).normal(0.0, 0.1, (n, 3))
    k = np.arange(max(n - 2, 0))
    f = np.stack([k, k + 1, k + 2], axis=1)
    f[k % 2 == 1] = f[k % 2 == 1][:, [1, 0, 2]]
    return v.astype(np.float32), f.astype(np.int32)


def class_cases():
    """name -> (verts, faces, fixed or None, {mode: the class of every vertex}): rule c by hand"""
    rng = np.random.default_rng(5)
    pts = lambda n: rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)
    c = {}
    c['single_triangle'] = (pts(3), [[0, 1, 2]], None, {0: [2, 2, 2], 1: [1, 1, 1], 2: [0, 0, 0]})
    # two triangles that share vertex 2 alone: it lies on four boundary edges
    c['bow_tie'] = (pts(5), [[0, 1, 2], [2, 3, 4]], None, {0: [2] * 5, 1: [1, 1, 2, 1, 1], 2: [0] * 5})
    # three faces on the edge (0, 1): its ends are non-manifold; the wing tips are on two boundary edges each
    c['three_on_an_edge'] = (pts(5), [[0, 1, 2], [1, 0, 3], [0, 1, 4]], None, {0: [3, 3, 2, 2, 2], 1: [3, 3, 1, 1, 1], 2: [0] * 5})
    # the same triangle twice: every edge has two faces, so nothing is a boundary
    c['duplicated_face'] = (pts(3), [[0, 1, 2], [0, 1, 2]], None, {0: [0, 0, 0], 1: [0, 0, 0], 2: [0, 0, 0]})
    tv, tf = tetrahedron()
    c['unreferenced_vertex'] = (np.concatenate([tv, pts(1)]), tf.tolist(), None, {m: [0, 0, 0, 0, 5] for m in (0, 1, 2)})
    # the mask wins over every other class, the unreferenced one included
    c['masked_vertex'] = (np.concatenate([tv, pts(1)]), tf.tolist(), [0, 1, 0, 0, 1], {m: [0, 4, 0, 0, 4] for m in (0, 1, 2)})
    return {k: (v, np.array(f, np.int32), None if fx is None else np.array(fx, np.uint8), want) for k, (v, f, fx, want) in c.items()}


def shuffled(faces, seed=0):
    """the faces in another order, every one with its corners rotated or flipped"""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces, np.int32)[rng.permutation(len(faces))]
    order = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])[rng.integers(0, 6, len(f))]
    return np.take_along_axis(f, order, axis=1)
