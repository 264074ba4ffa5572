"""CPU models of p2s_mesh_voxelize (include/p2s_hip.h, "next" row f-9), and the meshes its tests are built on.

``exact`` is independent of the kernel's method: exact rationals (fractions.Fraction) on the float32 coordinates; per voxel
centre "on the surface" (exact point-in-triangle), else the integer winding number from the crossings of a ray whose
direction is tried until no crossing is degenerate.

``kernel`` restates the kernel's rules operation for operation in numpy float64 (orient2 on x and y, orient3 = ((b - a) x
(c - a)) . (d - a) with dot3 = (x + y) + z, the filter bounds with S' = max(S, 1)): it gives the expected flags and report,
and the occupancy of every voxel the rules decide."""
from fractions import Fraction

import numpy as np

REPORT_KEYS = ('inside', 'undecided_columns', 'undecided_voxels', 'fallback', 'tests', 'crossings')
DIRECTIONS = ((3, 5, 7), (-7, 3, 5), (5, -7, 3), (1, 2, -9), (11, -2, 3), (2, 13, -5))


def centres(res):
    """the voxel centres of one axis: the float32 nearest to ((i + 0.5) / res) * 2 - 1 evaluated in float64"""
    return ((np.arange(res, dtype=np.float64) + 0.5) / np.float64(res) * 2.0 - 1.0).astype(np.float32)


# ---- meshes
def cube(half, centre=(0.0, 0.0, 0.0), inward=False):
    """an axis cube of 12 faces, outward (or inward) oriented; every face's diagonal runs through its (-, -) corner"""
    h, c = np.float32(half), np.asarray(centre, np.float32)
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * h + c
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int32)
    return v, (f[:, ::-1].copy() if inward else f)


def octahedron(radius):
    r = np.float32(radius)
    v = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def join(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def cube_with_cavity():
    return join(cube(0.4), cube(0.2, inward=True))


def two_cubes():
    """two outward cubes of half-side 0.3 centred at x = -0.15 and x = +0.15: the overlap |x| < 0.15 has w = 2"""
    return join(cube(0.3, (-0.15, 0.0, 0.0)), cube(0.3, (0.15, 0.0, 0.0)))


def open_cube(half):
    v, f = cube(half)
    return v, f[:-1].copy()


def stored(verts, faces):
    """the triangles [F, 3, 3] float64 as the handle stores them: flipped when the signed volume is negative"""
    T = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces)]
    vol = np.einsum('ij,ij->i', T[:, 0], np.cross(T[:, 1], T[:, 2])).sum()
    return T[:, [0, 2, 1]] if vol < 0 else T


# ---- the exact model
def _frac(x):
    return Fraction(float(x))


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _edge_sides(tri, n, q):
    """the three edge functions of the point q (in the plane of tri), positive inside"""
    return [_dot(_cross(_sub(tri[(k + 1) % 3], tri[k]), _sub(q, tri[k])), n) for k in range(3)]


def exact_point(tris, normals, p):
    """(on_surface, winding number) of the point p (Fractions) against the triangles (Fractions)"""
    for tri, n in zip(tris, normals):
        if _dot(n, _sub(p, tri[0])) == 0 and min(_edge_sides(tri, n, p)) >= 0:
            return True, 0
    for d in DIRECTIONS:
        w, ok = 0, True
        for tri, n in zip(tris, normals):
            den = _dot(n, d)
            num = _dot(n, _sub(tri[0], p))
            if den == 0:
                if num == 0:                      # the ray runs in the face's plane
                    ok = False
                    break
                continue
            t = num / den
            if t < 0:
                continue
            q = (p[0] + t * d[0], p[1] + t * d[1], p[2] + t * d[2])
            e = _edge_sides(tri, n, q)
            if min(e) < 0:
                continue
            if min(e) == 0 or t == 0:             # through an edge or a vertex
                ok = False
                break
            w += 1 if den > 0 else -1
        if ok:
            return False, w
    raise RuntimeError('every direction met an edge')


def exact(verts, faces, res):
    """(winding [res, res, res] int64, on_surface [res, res, res] bool) at the voxel centres, x-major with z fastest"""
    T = stored(verts, faces)
    tris = [[tuple(_frac(x) for x in corner) for corner in tri] for tri in T]
    normals = [_cross(_sub(t[1], t[0]), _sub(t[2], t[0])) for t in tris]
    if any(n == (0, 0, 0) for n in normals):
        raise ValueError('the exact model takes no zero-area face')
    c = [_frac(x) for x in centres(res)]
    w = np.zeros((res, res, res), np.int64)
    on = np.zeros((res, res, res), bool)
    for i in range(res):
        for j in range(res):
            for k in range(res):
                on[i, j, k], w[i, j, k] = exact_point(tris, normals, (c[i], c[j], c[k]))
    return w, on


# ---- the kernel's rules in float64
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def orient3(a, b, c, d):
    return dot3(cross3(b - a, c - a), d - a)


def orient2(a, b, c):
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])


def sgn(x, eps):
    return (x > eps).astype(np.int64) - (x < -eps).astype(np.int64)


def winding_sum(T, p):
    """the generalised winding number of the points p [n, 3] (van Oosterom & Strackee), float64"""
    a, b, c = (T[None, :, k] - p[:, None] for k in range(3))
    la, lb, lc = (np.sqrt(dot3(x, x)) for x in (a, b, c))
    num = dot3(a, cross3(b, c))
    den = ((la * lb * lc + dot3(a, b) * lc) + dot3(b, c) * la) + dot3(c, a) * lb
    return np.arctan2(num, den).sum(1) / (2.0 * np.pi)


def kernel(verts, faces, res):
    """dict: occ [res, res, res] uint8, flags [res, res, res] uint8, report (REPORT_KEYS; tests = those of method 1)"""
    T = stored(verts, faces)
    F = len(T)
    S = max(np.abs(T).max(), 1.0)
    eps2, eps3 = (S * S) * 2.0 ** -47, ((S * S) * S) * 2.0 ** -43
    c = centres(res).astype(np.float64)
    P = np.stack(np.meshgrid(c, c, indexing='ij'), -1).reshape(-1, 1, 2)           # [cols, 1, 2]
    A, B, C = (T[None, :, k, :2] for k in range(3))                               # [1, F, 2]
    lo, hi = T[:, :, :2].min(1)[None], T[:, :, :2].max(1)[None]
    inbox = ((P >= lo) & (P <= hi)).all(-1)
    s = np.stack([sgn(orient2(B, C, P), eps2), sgn(orient2(C, A, P), eps2), sgn(orient2(A, B, P), eps2)], -1)
    sigma = sgn(orient2(A, B, C), eps2)                                           # [1, F]
    miss = ~inbox | ((s > 0).any(-1) & (s < 0).any(-1))
    cross = ~miss & (sigma != 0) & (s == sigma[..., None]).all(-1)
    ucol = (~miss & ~cross).any(1)                                                # [cols]
    p = np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(res * res, res, 1, 3)
    side = sgn(orient3(T[None, None, :, 0], T[None, None, :, 1], T[None, None, :, 2], p), eps3) * sigma[:, None]      # [cols, res, F]
    live = cross[:, None, :] & ~ucol[:, None, None]
    single = (live & (side == 0)).any(-1)                                         # [cols, res]
    w = np.where(live & (side < 0), sigma[:, None], 0).sum(-1)
    flags = single | ucol[:, None]
    occ = (~flags & (w != 0)).astype(np.uint8)
    inside = int(occ.sum())
    if flags.any():
        wf = winding_sum(T, p.reshape(-1, 3)[flags.reshape(-1)])
        fb = np.abs(wf) > 0.5
        occ.reshape(-1)[np.flatnonzero(flags.reshape(-1))[fb]] = 1
        inside += int(fb.sum())
    report = dict(inside=inside, undecided_columns=int(ucol.sum()), undecided_voxels=int(single.sum()),
                  fallback=int(ucol.sum()) * res + int(single.sum()), tests=res * res * F, crossings=int(cross.sum()))
    return dict(occ=occ.reshape(res, res, res), flags=flags.astype(np.uint8).reshape(res, res, res), report=report)
