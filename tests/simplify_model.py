"""float64 numpy model of points2surf_amd.simplify (include/p2s_hip.h: p2s_mesh_simplify): quadric vertex
clustering, steps a-h of the definition with the same operations in the same order -- the grid of the voxel thinning, the
search over R, the smallest ids, the sums of a cell in ascending vertex / face id -- so that the discrete outputs and the
mean placement of the device must equal these, and the quadric placement to one float32 ulp.  The quadric solve is
``numpy.linalg.solve`` on A + eps tr(A) I: an independent solver (the device factorises by Cholesky).

Also the meshes that the CPU and the GPU tests share.
"""
import numpy as np

DEGENERATE_REL = 2.0 ** -90


def _f32(verts):
    return np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))


def _i32(faces):
    return np.ascontiguousarray(np.asarray(faces).astype(np.int32).reshape(-1, 3))


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


# ---- b. the grid (tests/prepare_model.py: voxel_cells) -------------------------------------------------------------------

def grid(verts, R):
    """(lo float64 [3], ext, h): the bounding box minimum of all vertices, its largest extent, the cell size"""
    p = _f32(verts)
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    ext = float((hi - lo).max())
    return lo, ext, ext / float(R)


def cells(verts, R):
    """(cell index per axis int64 [V, 3], linear cell id int64 [V])"""
    p = _f32(verts)
    lo, ext, _ = grid(p, R)
    scale = float(R) / ext if ext > 0.0 else 0.0
    ia = np.minimum(np.floor((p.astype(np.float64) - lo) * scale), float(R - 1)).astype(np.int64)
    return ia, (ia[:, 0] * R + ia[:, 1]) * R + ia[:, 2]


def surviving_mask(verts, faces, R):
    """c: the faces whose three corners lie in three pairwise different cells"""
    f = _i32(faces)
    lin = cells(verts, R)[1]
    a, b, c = lin[f[:, 0]], lin[f[:, 1]], lin[f[:, 2]]
    return (a != b) & (b != c) & (c != a)


def surviving(verts, faces, R):
    return int(surviving_mask(verts, faces, R).sum())


def search_resolution(verts, faces, max_faces, count=None):
    """(R, probes): the loop that defines R (surviving(R) is not monotone over grids that do not nest)"""
    count = count or (lambda R: surviving(verts, faces, R))
    lo, hi, probes = 1, 1024, 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        probes += 1
        if count(mid) <= max_faces:
            lo = mid
        else:
            hi = mid - 1
    return lo, probes


# ---- the report's words ----------------------------------------------------------------------------------------------------

def edge_word(faces):
    """boundary edges | edges of more than two faces << 32: undirected edges by the number of faces' sides on them"""
    f = _i32(faces).astype(np.int64)
    if f.shape[0] == 0:
        return 0
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = (e.min(axis=1) << 32) | e.max(axis=1)
    n = np.unique(key, return_counts=True)[1]
    return int((n == 1).sum()) | (int((n > 2).sum()) << 32)


def degenerate_mask(verts, faces):
    """|ab x ac|^2 <= 2^-90 |ab|^2 |ac|^2 on the stored coordinates"""
    p, f = _f32(verts).astype(np.float64), _i32(faces)
    ab, ac = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    n = _cross(ab, ac)
    return ~(_dot(n, n) > DEGENERATE_REL * (_dot(ab, ab) * _dot(ac, ac)))


def _ordered_sums(seg, vals, n):
    """[n, k]: the rows of vals [N, k] added per segment front to back, starting from 0 (seg [N] ascending)"""
    out = np.zeros((n, vals.shape[1]))
    start = np.searchsorted(seg, np.arange(n), 'left')
    count = np.searchsorted(seg, np.arange(n), 'right') - start
    for k in range(int(count.max()) if n else 0):
        sel = np.nonzero(count > k)[0]
        out[sel] = out[sel] + vals[start[sel] + k]
    return out, count


# ---- a-h --------------------------------------------------------------------------------------------------------------------

def simplify(verts, faces, max_faces=100000, resolution=0, placement='quadric', epsilon=1e-3):
    """dict: verts float32 [V', 3], faces int32 [F', 3], face_src int32 [F'], vert_map int32 [V], report int64 [16],
    centre float64 [V', 3] (the cell centres g), h, ratio float64 [V'] (max |x| / h of the quadric minimiser before the
    fallback decides; nan where no solve ran), m float64 [V', 3] (the means relative to g)"""
    p, f = _f32(verts), _i32(faces)
    V, F = p.shape[0], f.shape[0]
    quadric = {'mean': False, 'quadric': True}[placement]
    rep = np.zeros(16, np.int64)
    rep[0] = V | (F << 32)
    rep[3] = resolution
    empty = dict(verts=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), face_src=np.zeros(0, np.int32),
                 vert_map=np.full(V, -1, np.int32), report=rep, centre=np.zeros((0, 3)), h=0.0, ratio=np.zeros(0),
                 m=np.zeros((0, 3)))
    if F == 0:
        return empty
    if V == 0 or f.min() < 0 or f.max() >= V or not np.isfinite(p).all():
        raise ValueError('index out of range or non-finite vertex')
    rep[13] = edge_word(f)
    R = int(resolution)
    if R == 0:
        if F <= max_faces:
            rep[1], rep[2], rep[12] = V, F, rep[13]
            return dict(empty, verts=p.copy(), faces=f.copy(), face_src=np.arange(F, dtype=np.int32),
                        vert_map=np.arange(V, dtype=np.int32))
        R, rep[11] = search_resolution(p, f, max_faces)
    rep[3] = R
    lo, ext, h = grid(p, R)
    idx, lin = cells(p, R)
    x64 = p.astype(np.float64)

    # c, d: the cells, their smallest vertex ids, the surviving faces, the cells with an output vertex
    _, first, inv = np.unique(lin, return_index=True, return_inverse=True)
    small = first[inv.reshape(-1)]                            # per vertex the smallest vertex id of its cell
    rep[4] = first.size
    w = small[f]
    keep = (w[:, 0] != w[:, 1]) & (w[:, 1] != w[:, 2]) & (w[:, 2] != w[:, 0])
    rep[5] = F - int(keep.sum())
    rep[7] = int(degenerate_mask(p, f).sum())
    used = np.zeros(V, bool)
    used[w[keep].reshape(-1)] = True
    out_of_small = np.cumsum(used) - 1                        # ordered by the smallest vertex id
    vert_map = np.where(used[small], out_of_small[small], -1).astype(np.int32)
    V1 = int(used.sum())

    # f: duplicates -- of the faces with one vertex set the smallest face id
    ids = np.nonzero(keep)[0]
    if ids.size:
        sets = np.sort(w[ids], axis=1)
        _, firsts = np.unique(sets, axis=0, return_index=True)
        ids = ids[np.sort(firsts)]
    rep[6] = int(keep.sum()) - ids.size
    faces_out = vert_map[f[ids]].astype(np.int32).reshape(-1, 3)
    rep[1], rep[2] = V1, ids.size
    rep[12] = edge_word(faces_out)
    if V1 == 0:
        return dict(empty, vert_map=vert_map, h=h)

    # e: the mean of a cell's vertices relative to its centre, in ascending vertex id
    centre_of_vertex = lo + (idx.astype(np.float64) + 0.5) * h
    members = np.nonzero(vert_map >= 0)[0]
    order = members[np.argsort(vert_map[members], kind='stable')]
    sums, count = _ordered_sums(vert_map[order], x64[order] - centre_of_vertex[order], V1)
    m = sums / count[:, None].astype(np.float64)
    g = centre_of_vertex[np.nonzero(used)[0]]                 # [V1, 3]
    x = m.copy()
    ratio = np.full(V1, np.nan)
    if quadric:
        deg = degenerate_mask(p, f)
        o = vert_map[f]                                       # [F, 3] output id of every corner's cell, -1: none
        emit = np.stack([o[:, 0] >= 0, (o[:, 1] >= 0) & (w[:, 1] != w[:, 0]),
                         (o[:, 2] >= 0) & (w[:, 2] != w[:, 0]) & (w[:, 2] != w[:, 1])], axis=1) & ~deg[:, None]
        fi, ci = np.nonzero(emit)
        cell = o[fi, ci].astype(np.int64)
        srt = np.lexsort((fi, cell))                          # by cell, then ascending face id
        fi, cell = fi[srt], cell[srt]
        a, b, c = (x64[f[fi, j]] - g[cell] for j in range(3))
        n = _cross(b - a, c - a)
        d = -_dot(n, a)
        vals = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2],
                         n[:, 2] * n[:, 2], d * n[:, 0], d * n[:, 1], d * n[:, 2]], axis=1)
        acc, _ = _ordered_sums(cell, vals, V1)
        A = acc[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(V1, 3, 3)
        r = acc[:, 6:9]
        tr = (acc[:, 0] + acc[:, 3]) + acc[:, 5]
        solve = tr != 0.0
        rep[9] = int((~solve).sum())
        if solve.any():
            M = A[solve] + (epsilon * tr[solve])[:, None, None] * np.eye(3)
            rhs = np.einsum('nij,nj->ni', A[solve], m[solve]) + r[solve]
            q = m[solve] - np.linalg.solve(M, rhs[:, :, None])[:, :, 0]
            big = np.abs(q).max(axis=1)
            ratio[solve] = big / h
            fallback = big > h
            q[fallback] = m[solve][fallback]
            x[solve] = q
            rep[10] = int(fallback.sum())
            rep[8] = int(solve.sum()) - rep[10]
    return dict(verts=(g + x).astype(np.float32), faces=faces_out, face_src=ids.astype(np.int32), vert_map=vert_map,
                report=rep, centre=g, h=h, ratio=ratio, m=m)


# ---- meshes -------------------------------------------------------------------------------------------------------------------

def rotation(seed=7):
    """a rotation with no axis near a coordinate axis"""
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def torus(nu=160, nv=64, R=0.35, r=0.14, seed=7):
    """a closed torus of nu x nv quads (2 nu nv faces), rotated so that nothing is axis-aligned"""
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing='ij')
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return (p @ rotation(seed).T).astype(np.float32), faces.astype(np.int32)


def cube(n=24):
    """the welded surface of the unit cube, n x n quads per side (12 n^2 faces, 6 n^2 + 2 vertices), outward"""
    t = np.arange(n + 1)
    i, j = np.meshgrid(t, t, indexing='ij')
    lattice, tris = [], []
    for axis in range(3):
        for side in (0, n):
            q = np.zeros((n + 1, n + 1, 3), np.int64)
            q[..., axis] = side
            q[..., (axis + 1) % 3] = i
            q[..., (axis + 2) % 3] = j
            base = sum(x.shape[0] for x in lattice)
            lattice.append(q.reshape(-1, 3))
            k = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1) + base
            a, b, c, d = k, k + (n + 1), k + (n + 1) + 1, k + 1
            quad = [np.stack([a, b, c], -1), np.stack([a, c, d], -1)]
            if side == 0:                                     # the normal of (a, b, c) is +axis
                quad = [t3[:, ::-1] for t3 in quad]
            tris += quad
    lattice = np.concatenate(lattice)
    uniq, inv = np.unique(lattice, axis=0, return_inverse=True)
    faces = inv.reshape(-1)[np.concatenate(tris)]
    return (uniq.astype(np.float64) / n).astype(np.float32), faces.astype(np.int32)


CUBE_CORNERS = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])


def corner_distances(verts, h):
    """for every corner of the unit cube the distance to the nearest vertex, in units of h"""
    d = np.linalg.norm(np.asarray(verts, np.float64)[None] - CUBE_CORNERS[:, None], axis=2).min(axis=1)
    return d / h
