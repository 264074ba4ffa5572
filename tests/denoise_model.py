"""The numpy model of DESIGN 4.8 f18 (include/p2s_hip.h: p2s_mesh_denoise, rules b to g), with no device: the same normals,
neighbours, classes, iterations and report, in the same float64 operations in the same order and with float32 storage between
iterations, so that the device is compared with it for EQUALITY of bytes.  The rows (the neighbours of a face, the live faces of
a vertex) are padded to the largest length of their bucket and visited column by column in a Python loop under a mask: the
sequential order of rules d and f.  The mesh builders are those of tests/smooth_model.py; the cube, the fan and the hand-made
class cases of this unit are added here."""
import numpy as np

import smooth_model as SM
from smooth_model import grid, icosphere, octahedron, tetrahedron      # noqa: F401  (the tests take them from here)

EINVAL = -1
FREE, BOUNDARY_FIXED, MASKED, UNREFERENCED, NO_LIVE_FACE = 0, 1, 2, 3, 4
MODES = {'fixed': 0, 'free': 1}


def face_normals(P, f):
    """rule b -> [F, 3] float32; a dead face has (0, 0, 0)"""
    p = np.asarray(P, np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        a = p[f[:, 0]]
        e1, e2 = p[f[:, 1]] - a, p[f[:, 2]] - a
        m = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        l = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        live = (l > 0) & np.isfinite(l)
        n = np.zeros((len(f), 3), np.float32)
        n[live] = (m[live] / l[live, None]).astype(np.float32)
    return n


def is_live(n):
    return np.any(n != 0, axis=1)


def vertex_rows(V, f, keep=None):
    """start [V + 1], col: the faces at every vertex, ascending; ``keep`` [F, 3] bool drops corners"""
    fid = np.repeat(np.arange(len(f), dtype=np.int64), 3)
    key = (f.reshape(-1) << 32) | fid
    if keep is not None:
        key = key[keep.reshape(-1)]
    key = np.sort(key)
    start = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(key >> 32, minlength=V), out=start[1:])
    return start, key & 0xffffffff


def neighbours(V, f):
    """rule c -> start [F + 1], col: N(i) of every face, itself included, each once, ascending"""
    F = len(f)
    vstart, vcol = vertex_rows(V, f)
    cv, cf = f.reshape(-1), np.repeat(np.arange(F, dtype=np.int64), 3)
    d = np.diff(vstart)[cv]
    first = np.cumsum(d) - d
    off = np.arange(int(d.sum()), dtype=np.int64) - np.repeat(first, d)
    key = np.unique((np.repeat(cf, d) << 32) | vcol[np.repeat(vstart[cv], d) + off])
    start = np.zeros(F + 1, np.int64)
    np.cumsum(np.bincount(key >> 32, minlength=F), out=start[1:])
    return start, key & 0xffffffff


def classes(V, f, live, mode, fixed=None):
    """rule e -> the class byte of every vertex"""
    a, b, cnt = SM.edges(f)
    one = cnt == 1
    bdeg = np.bincount(a[one], minlength=V) + np.bincount(b[one], minlength=V)
    cls = np.zeros(V, np.uint8)
    if mode == 0:
        cls[bdeg > 0] = BOUNDARY_FIXED
    cls[np.bincount(f[live].reshape(-1), minlength=V) == 0] = NO_LIVE_FACE
    cls[np.bincount(f.reshape(-1), minlength=V) == 0] = UNREFERENCED
    if fixed is not None:
        cls[np.asarray(fixed).reshape(-1) != 0] = MASKED
    return cls


def normal_step(N, blocks, T):
    """rule d on float32 normals N [F, 3] -> the next float32 normals"""
    out = N.copy()
    T = np.float64(T)
    with np.errstate(all='ignore'):
        for ids, nb, mask, _ in blocks:
            ni = N[ids].astype(np.float64)
            s = np.zeros((len(ids), 3), np.float64)
            for k in range(nb.shape[1]):                               # the order of the sum: ascending j
                nj = N[nb[:, k]].astype(np.float64)
                d = (ni[:, 0] * nj[:, 0] + ni[:, 1] * nj[:, 1]) + ni[:, 2] * nj[:, 2]
                w = (d - T) * (d - T)
                s = np.where((mask[:, k] & (d > T))[:, None], s + w[:, None] * nj, s)
            l = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
            ok = (l > 0) & np.isfinite(l) & is_live(N[ids])
            out[ids[ok]] = (s[ok] / l[ok, None]).astype(np.float32)
    return out


def vertex_step(P, f, N, blocks):
    """rule f on float32 positions P [V, 3] with the target normals N -> the next float32 positions"""
    Q = P.copy()
    with np.errstate(all='ignore'):
        for ids, tab, mask, k in blocks:
            p = P[ids].astype(np.float64)
            s = np.zeros((len(ids), 3), np.float64)
            for c in range(tab.shape[1]):                              # the order of the sum: ascending face
                fc = f[tab[:, c]]
                g = ((P[fc[:, 0]].astype(np.float64) + P[fc[:, 1]].astype(np.float64)) + P[fc[:, 2]].astype(np.float64)) / 3.0
                n = N[tab[:, c]].astype(np.float64)
                e = g - p
                d = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
                s = np.where(mask[:, c, None], s + n * d[:, None], s)
            Q[ids] = (p + s / k.astype(np.float64)[:, None]).astype(np.float32)
    return Q


def denoise(verts, faces, threshold=0.5, normal_iterations=10, vertex_iterations=10, mode=0, fixed=None):
    """p2s_mesh_denoise: dict(rc, verts [V, 3] float32, normals [F, 3] float32, cls [V] uint8, report [16] int64)"""
    P0 = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(P0), len(f)
    N = face_normals(P0, f)
    live = is_live(N)
    cls = classes(V, f, live, mode, fixed)
    rep = np.zeros(16, np.int64)
    rep[0] = V | (F << 32)
    rep[1:6] = np.bincount(cls, minlength=5)
    rep[6] = int((~live).sum())
    if live.any():
        fstart, fcol = neighbours(V, f)
        rep[7] = int(np.diff(fstart)[live].max())
        rep[8] = normal_iterations
        blocks = SM._blocks(fstart, fcol)
        for _ in range(normal_iterations):
            N = normal_step(N, blocks, threshold)
    P = P0
    if (cls == FREE).any():
        rep[9] = vertex_iterations
        vstart, vcol = vertex_rows(V, f, keep=live[:, None] & (cls[f] == FREE))
        blocks = SM._blocks(vstart, vcol)
        for _ in range(vertex_iterations):
            P = vertex_step(P, f, N, blocks)
    fin = np.isfinite(P)
    with np.errstate(all='ignore'):
        dd = P.astype(np.float64) - P0.astype(np.float64)
        dsq = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    ok = fin.all(axis=1)
    rep[10] = np.array([dsq[ok].max() if ok.any() else 0.0], np.float64).view(np.int64)[0]
    rep[11] = int((~fin).sum())
    return dict(rc=EINVAL if rep[11] else 0, verts=P, normals=N, cls=cls, report=rep)


def normal_error_deg(v, f, v_clean):
    """the mean angle in degrees between the face normals of (v, f) and those of (v_clean, f), in float64"""
    def unit(p):
        p = np.asarray(p, np.float64)[np.asarray(f, np.int64)]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        return n / np.linalg.norm(n, axis=1)[:, None]
    return float(np.degrees(np.arccos(np.clip(np.einsum('ij,ij->i', unit(v), unit(v_clean)), -1.0, 1.0))).mean())


# ---- meshes
def cube(n):
    """the unit cube, n x n quads per side, two outward triangles per quad, welded: 6 n^2 + 2 vertices, 12 n^2 faces (float64)"""
    index, faces = {}, []

    def vid(p):
        return index.setdefault(p, len(index))
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3                           # e_u x e_w = e_axis
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for du, dw in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        q = [0, 0, 0]
                        q[axis], q[u], q[w] = side, i + du, j + dw
                        quad.append(vid(tuple(q)))
                    if side == 0:
                        quad.reverse()
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    v = np.array(sorted(index, key=index.get), np.float64) / n
    return v, np.array(faces, np.int32)


def noisy_cube(n, seed=3, rel=0.2):
    """cube(n) with RandomState(seed).normal(0, rel / n) on every coordinate -> noisy float32 vertices, faces, clean vertices"""
    v, f = cube(n)
    return (v + np.random.RandomState(seed).normal(0.0, rel / n, v.shape)).astype(np.float32), f, v.astype(np.float32)


def fan(n, seed=0):
    """an apex (vertex 0) over a closed ring of n vertices: n faces that are all neighbours of each other"""
    a = 2.0 * np.pi * np.arange(n) / n
    rng = np.random.default_rng(seed)
    ring = np.stack([np.cos(a), np.sin(a), rng.normal(0.0, 0.05, n)], axis=1)
    v = np.concatenate([[[0.02, -0.01, 0.6]], ring])
    i = np.arange(n)
    return v.astype(np.float32), np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1).astype(np.int32)


def class_cases():
    """name -> (verts, faces, fixed or None, {mode: the class of every vertex}): rule e by hand"""
    rng = np.random.default_rng(6)
    pts = lambda n: rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)
    c = {}
    gv, gf = grid(3, 3, noise=0.1, seed=1)                              # an open sheet: the middle vertex alone is inside
    c['open_sheet'] = (gv, gf.tolist(), None, {0: [1, 1, 1, 1, 0, 1, 1, 1, 1], 1: [0] * 9})
    tv, tf = tetrahedron()
    tv = tv + rng.normal(0.0, 0.1, tv.shape).astype(np.float32)
    c['masked_vertices'] = (np.concatenate([tv, pts(1)]), tf.tolist(), [0, 1, 0, 0, 1], {m: [0, 2, 0, 0, 2] for m in (0, 1)})
    c['unreferenced_vertex'] = (np.concatenate([tv, pts(1)]), tf.tolist(), None, {m: [0, 0, 0, 0, 3] for m in (0, 1)})
    # the face (4, 5, 6) has three distinct collinear corners: dead, and its vertices have no live face
    line = np.array([[3, 0, 0], [4, 0, 0], [6, 0, 0]], np.float32)
    c['all_faces_dead'] = (np.concatenate([tv, line]), tf.tolist() + [[4, 5, 6]], None, {m: [0, 0, 0, 0, 4, 4, 4] for m in (0, 1)})
    # a dead face on vertex 0 of the tetrahedron: 0 keeps its live faces, and in mode 0 it lies on an edge of one face
    ray = np.stack([tv[0] * np.float32(2), tv[0] * np.float32(4)])
    c['dead_face_on_a_live_vertex'] = (np.concatenate([tv, ray]), tf.tolist() + [[0, 4, 5]], None,
                                       {0: [1, 0, 0, 0, 4, 4], 1: [0, 0, 0, 0, 4, 4]})
    return {k: (np.asarray(v, np.float32), np.array(f, np.int32), None if fx is None else np.array(fx, np.uint8), want)
            for k, (v, f, fx, want) in c.items()}
