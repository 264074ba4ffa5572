"""TEST INFRASTRUCTURE ONLY -- plain models of the mesh-metric kernels (points2surf_amd/csrc/p2s_metrics.hip) and the
inputs that aim at their mechanisms.  numpy and Python only: brute force over all pairs, an explicit binary search, the
documented rules written down once more.  Independent of oracle/metrics_oracle.py (scipy's trees + the trimesh
restatement), against which tests/test_metrics_model.py pins every function here; tests/test_gpu_metrics_edges.py then
holds the device to both.

Every distance is the float64 value of the float32 coordinates, summed as (dx*dx + dy*dy) + dz*dz -- the association of
the kernels (contraction off) and of scipy's squared-Euclidean loop, so that equal inputs give equal bits."""
import math

import numpy as np

SENTINEL = np.float32(-7777.25)          # fills output rows the device must not touch


def _f64(points):
    return np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3)).astype(np.float64)


def _d2_block(a, b):
    """[len(a), len(b)] squared distances, (dx*dx + dy*dy) + dz*dz"""
    dx = a[:, 0:1] - b[None, :, 0]
    dy = a[:, 1:2] - b[None, :, 1]
    dz = a[:, 2:3] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


# ---- models ------------------------------------------------------------------------------------------------------------

def close_pairs(points_f32, radius):
    """all (i, j), i < j, with squared distance <= radius * radius, in lexicographic order; brute force"""
    p = _f64(points_f32)
    r2 = float(radius) * float(radius)
    out = []
    for i0 in range(0, len(p), 512):
        d2 = _d2_block(p[i0:i0 + 512], p)
        i, j = np.nonzero(d2 <= r2)
        i = i + i0
        sel = j > i
        out.append(np.stack([i[sel], j[sel]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def remove_close_model(points_f32, radius):
    """trimesh.points.remove_close as the kernels state it -> (keep_mask, degree): degree = the number of close partners
    (squared distance <= radius * radius); of every close pair i < j the point i goes if degree[i] >= degree[j], else j"""
    m = len(_f64(points_f32))
    pairs = close_pairs(points_f32, radius)
    degree = np.bincount(pairs.ravel(), minlength=m).astype(np.int64)
    keep = np.ones(m, dtype=bool)
    if len(pairs):
        i, j = pairs[:, 0], pairs[:, 1]
        keep[np.where(degree[i] >= degree[j], i, j)] = False
    return keep, degree


def nn_model(queries_f32, targets_f32, chunk=2048):
    """-> (dist [n] float64 = sqrt(min over the targets of d2), their max, their sum by math.fsum); chunked brute force"""
    q, t = _f64(queries_f32), _f64(targets_f32)
    dist = np.empty(len(q), dtype=np.float64)
    for i0 in range(0, len(q), chunk):
        dist[i0:i0 + chunk] = np.sqrt(_d2_block(q[i0:i0 + chunk], t).min(axis=1))
    return dist, float(dist.max()), math.fsum(dist.tolist())


def face_areas(verts, faces):
    """|cross(v1 - v0, v2 - v0)| / 2 in float64 from the float32 vertices, squares summed as (x + y) + z"""
    v = _f64(verts)
    f = np.asarray(faces).reshape(-1, 3)
    a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return np.sqrt((cx * cx + cy * cy) + cz * cz) * 0.5


def searchsorted_left(cum, pick):
    """the first index with cum[index] >= pick (len(cum) if none), by bisection, for every pick"""
    cum = np.asarray(cum, dtype=np.float64)
    out = np.empty(len(pick), dtype=np.int64)
    for n, x in enumerate(np.asarray(pick, dtype=np.float64).tolist()):
        lo, hi = 0, len(cum)
        while lo < hi:
            mid = (lo + hi) >> 1
            if cum[mid] < x:
                lo = mid + 1
            else:
                hi = mid
        out[n] = lo
    return out


def sample_model(verts, faces, u, cum=None):
    """trimesh.sample.sample_surface from given deviates u = [n picks | n length pairs, row-major]:
    face = min(searchsorted_left(cum, pick * cum[-1]), nf - 1); lengths (l1, l2) with l1 + l2 > 1 become |l - 1|;
    point = (e1 * l1 + e2 * l2) + v0 in float64, rounded once to float32.
    -> (points [n, 3] float32, faces [n] int64, area = cum[-1], cum float64 = np.cumsum of the face areas)"""
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    n = len(u) // 3
    assert len(u) == 3 * n
    v = _f64(verts)
    f = np.asarray(faces).reshape(-1, 3)
    if cum is None:
        cum = np.cumsum(face_areas(verts, faces))
    face = np.minimum(searchsorted_left(cum, u[:n] * cum[-1]), len(cum) - 1)
    l1, l2 = u[n::2].copy(), u[n + 1::2].copy()
    fold = l1 + l2 > 1.0
    l1[fold] = np.abs(l1[fold] - 1.0)
    l2[fold] = np.abs(l2[fold] - 1.0)
    o = v[f[face, 0]]
    e1, e2 = v[f[face, 1]] - o, v[f[face, 2]] - o
    pts = ((e1 * l1[:, None] + e2 * l2[:, None]) + o).astype(np.float32)
    return pts, face, float(cum[-1]), cum


def boundary_margin(cum, u_picks):
    """for every pick u * cum[-1] its distance to the nearest cumulative value (the decision boundaries of searchsorted)"""
    cum = np.asarray(cum, dtype=np.float64)
    pick = np.asarray(u_picks, dtype=np.float64) * cum[-1]
    k = np.searchsorted(cum, pick)
    above = np.abs(cum[np.minimum(k, len(cum) - 1)] - pick)
    below = np.where(k > 0, np.abs(pick - cum[np.maximum(k - 1, 0)]), np.inf)
    return np.minimum(above, below)


# ---- recipes -----------------------------------------------------------------------------------------------------------

LEGS = (1, 2, 3, 5)                      # in units of 2^-8: areas a * b * 2^-17, a, b in LEGS


def degenerate_positions(nf):
    """the standard places of zero-area faces in lattice_mesh(nf): first, last, 1023 and 1024 (the seam of the scan's
    first chunk), and two runs; always leaves faces with area.  {} for nf == 1."""
    if nf < 2:
        return {}
    want = [0] if nf == 2 else [0, nf - 1, 1023, 1024]
    if nf >= 63:
        want += list(range(nf // 3, nf // 3 + 5)) + list(range(2 * nf // 3, 2 * nf // 3 + 2))
    pos = sorted(set(p for p in want if 0 <= p < nf))
    return dict((p, 'repeat' if n % 2 == 0 else 'collinear') for n, p in enumerate(pos))


def lattice_mesh(nf, degenerate_at=None):
    """Aims at scan_f64_kernel (carry across chunks of 1024, wave bases) and at mesh_sample_kernel's searchsorted-left
    rule over repeated cumulative values.  A planar mesh (z = 0.25) of nf axis-aligned right triangles, three vertices
    each, every coordinate a multiple of 2^-8, legs a * 2^-8 and b * 2^-8 with a, b cycling through LEGS with different
    periods, the right angle at v0, v1 or v2 in turn and both orientations.  Every area is a * b * 2^-17 exactly and every
    partial sum of up to 2^20 of them, in any order, is exact in float64 (an integer below 2^25 times 2^-17): no
    association of the additions can change a bit of the cumulative areas, so the device's face picks must agree with
    np.cumsum's for every sample.  ``degenerate_at``: {face index: 'repeat' | 'collinear'} -- faces of area exactly 0, by
    a repeated vertex (v2 = v1) or by three collinear vertices (v2 = v0 + 2 (v1 - v0)); they repeat a cumulative value
    and must never be picked by a deviate > 0.  -> (verts [3 nf, 3] float32, faces [nf, 3] int32)"""
    degenerate_at = degenerate_at or {}
    h = 2.0 ** -8
    verts = np.zeros((3 * nf, 3), dtype=np.float64)
    faces = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3).copy()
    for f in range(nf):
        a = LEGS[f % 4] * h * (1 if (f // 5) % 2 == 0 else -1)
        b = LEGS[(f // 4 + f // 7) % 4] * h
        corner = np.array([(f % 64) * 16 * h + 8 * h, (f // 64) * 16 * h + 8 * h, 0.25])
        px, py = corner + [a, 0.0, 0.0], corner + [0.0, b, 0.0]
        tri = [(corner, px, py), (py, corner, px), (px, py, corner)][f % 3]      # the right angle at v0, v1, v2
        kind = degenerate_at.get(f)
        if kind == 'repeat':
            faces[f, 2] = faces[f, 1]            # the same vertex index twice (its third vertex stays, unused)
        elif kind == 'collinear':
            tri = (tri[0], tri[1], tri[0] + 2.0 * (tri[1] - tri[0]))
        elif kind is not None:
            raise ValueError(kind)
        verts[3 * f:3 * f + 3] = tri
    v32 = verts.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), verts)
    return v32, faces


def lattice_points(n_side, h, m=None, seed=0):
    """Aims at the `<= r2` comparison and the tie rule of close_degree_kernel / close_remove_kernel.  The n_side^3 points
    0.25 + h * (i, j, k), h a power of two, in a seeded random order (so that neighbours sit in different 256-point
    tiles), cut to the first m.  Differences, squares and their sums are exact, so at radius h (6 partners inside) and 2h
    (32 partners) the outermost partners lie EXACTLY at the radius and count only because the comparison is `<=`; inner
    points all have the same degree, so most pairs are decided by the tie rule.  -> [m, 3] float32"""
    g = np.arange(n_side, dtype=np.float64) * h + 0.25
    p = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    p = p[np.random.RandomState(seed).permutation(len(p))]
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p)
    return p32 if m is None else p32[:m]


def lattice_side(m):
    """the smallest lattice with at least m points"""
    n = 1
    while n ** 3 < m:
        n += 1
    return n


def uniform_points(m, seed=5):
    """the input of the older test at any m: uniform in the unit cube (degrees up to ~5 at r = 0.03)"""
    return np.random.RandomState(seed).random_sample((m, 3)).astype(np.float32)


def clustered_points(m, seed=11):
    """Aims at degrees in the hundreds (int counters across many LDS tiles, the tie rule among high degrees) and at
    d2 == 0.  40 % of the points in a Gaussian cluster of sigma 0.006 (most of them mutually within r = 0.02), 10 % in
    stacks of five exact duplicates of uniform points, the rest uniform in the unit cube; seeded random order, so that
    the cluster is spread over all tiles.  -> ([m, 3] float32, is_stack [m] bool)"""
    rs = np.random.RandomState(seed)
    n_cluster, n_stack = (2 * m) // 5, (m // 10) // 5 * 5
    cluster = 0.5 + 0.006 * rs.standard_normal((n_cluster, 3))
    stacks = np.repeat(rs.random_sample((n_stack // 5, 3)), 5, axis=0)
    uniform = rs.random_sample((m - n_cluster - n_stack, 3))
    p = np.concatenate([cluster, stacks, uniform]).astype(np.float32)
    is_stack = np.zeros(m, dtype=bool)
    is_stack[n_cluster:n_cluster + n_stack] = True
    order = rs.permutation(m)
    return p[order], is_stack[order]


STRADDLE_RADIUS = 2.0 ** -6


def straddling_points(m):
    """Aims at the 256-point LDS tiles of close_degree_kernel / close_remove_kernel: the partial last tile (`lim`), the
    first tile a block of close_remove_kernel visits, the pairing of the first point with the last.  Point i at
    (i % 16, i // 16 % 16, i // 256): a unit lattice, everything far apart.  Then groups of points are moved next to
    each other (2^-7 apart along x, y; the radius is 2^-6): (0, m-1), (255, 256), every (256 t - 1, 256 t), and two
    points inside the last tile.  A point wanted by two pairs joins them into a group of three, mutually close.
    -> (points [m, 3] float32, pairs [[i, j]] i < j: every close pair, sorted, radius)"""
    i = np.arange(m)
    p = np.stack([i % 16, i // 16 % 16, i // 256], axis=1).astype(np.float64)
    want = [(0, m - 1), (255, 256)] + [(256 * t - 1, 256 * t) for t in range(2, (m + 255) // 256 + 1)]
    tile0 = (m - 1) // 256 * 256
    want.append((tile0 + 1, m - 2))
    group = {}                                   # point -> list of its group's members (shared)
    offsets = [np.zeros(3), np.array([2.0 ** -7, 0, 0]), np.array([0, 2.0 ** -7, 0])]
    for a, b in want:
        if not (0 <= a < b < m):
            continue
        ga, gb = group.get(a), group.get(b)
        if ga is None and gb is None:
            group[a] = group[b] = [a, b]
        elif ga is not None and gb is None and len(ga) < 3:
            ga.append(b)
            group[b] = ga
        elif gb is not None and ga is None and len(gb) < 3:
            gb.append(a)
            group[a] = gb
    pairs = set()
    for members in group.values():
        for n, k in enumerate(members):
            p[k] = p[members[0]] + offsets[n]
        for a in members:
            for b in members:
                if a < b:
                    pairs.add((a, b))
    return p.astype(np.float32), np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2), STRADDLE_RADIUS


def outlier_sets():
    """Aims at the query far outside the target's box, the one that decides a Hausdorff distance, with answers that need
    no model.  -> list of (name, A, B, (max A->B, sum A->B, max B->A, sum B->A)), all exact.
    'shifted lattice': A = 4^3 points h (i, j, k), h = 2^-3; B = A + (2^-4, 0, 0) and one point (3, 4, 0) * 2^-2 away from
    A's corner (3h, 3h, 3h).  Every a has a b exactly 2^-4 away (two of them: a nearest-id tie) -> max 2^-4, sum 64 * 2^-4
    = 4; every shifted b is 2^-4 from A and the outlier is 5 * 2^-2 = 1.25 from the corner, its nearest -> max 1.25, sum
    5.25.  All terms are multiples of 2^-4: any order of summation gives these bits.
    'copies': A = 3000 copies of c = (0.5, 0.25, 0.125); B = {c, c + (0, 3, 4) / 2}.  A -> B: 0, 0; B -> A: 2.5, 2.5."""
    h = 2.0 ** -3
    g = np.arange(4, dtype=np.float64) * h
    a = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    b = np.concatenate([a + [2.0 ** -4, 0, 0], [[3 * h + 0.75, 3 * h + 1.0, 3 * h]]])
    c = np.array([0.5, 0.25, 0.125])
    return [('shifted lattice', a.astype(np.float32), b.astype(np.float32), (0.0625, 4.0, 1.25, 5.25)),
            ('copies', np.tile(c, (3000, 1)).astype(np.float32), np.stack([c, c + [0, 1.5, 2.0]]).astype(np.float32),
             (0.0, 0.0, 2.5, 2.5))]


def fed_deviates(cum):
    """Aims at mesh_sample_kernel's edges with hand-written deviates for a mesh with cumulative areas ``cum``.
    Picks: 0.0; the largest double below 1; 0.5; and for many k a u with u * cum[-1] == cum[k] EXACTLY (found by
    trying cum[k] / cum[-1] and its neighbours; -> exact_k says which k were hit).  Length pairs: sums of exactly 1.0
    (not folded), the sum 1 + 2^-53 that rounds to 1.0 (not folded), 1 + 2^-52 (one ulp above: folded), both zero, and
    sums well above 1; the pairs at the limit are lopsided (0.25, 0.75), so that the fold moves the point across the
    triangle.  Every pick meets every length pair.  -> (u [3 n], exact_k [list], n)"""
    total = cum[-1]
    picks, exact_k = [0.0, 1.0 - 2.0 ** -53, 0.5], []
    for k in range(len(cum) - 1):
        if cum[k] <= 0.0:
            continue
        u0 = cum[k] / total
        for u in (u0, np.nextafter(u0, 0.0), np.nextafter(u0, 1.0)):
            if 0.0 < u < 1.0 and u * total == cum[k]:
                picks.append(float(u))
                exact_k.append(k)
                break
    lengths = [(0.25, 0.75), (0.5, 0.5), (2.0 ** -30, 1.0 - 2.0 ** -30), (0.25, 0.75 + 2.0 ** -53), (0.25, 0.75 + 2.0 ** -52),
               (0.75 + 2.0 ** -52, 0.25), (0.0, 0.0), (0.75, 0.75), (1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53), (0.0, 1.0 - 2.0 ** -53)]
    pk = np.repeat(np.array(picks, dtype=np.float64), len(lengths))
    ln = np.tile(np.array(lengths, dtype=np.float64), (len(picks), 1))
    return np.concatenate([pk, ln.reshape(-1)]), exact_k, len(pk)


def nn_targets():
    """name -> target cloud [nt, 3] float32 for the nearest-neighbour statistics: the smallest clouds (the cell grid is
    4^3 from one point on), a cloud with no extent, one with no extent in z, one with cells of hundreds of points and
    duplicates, and a lattice (nearest-id ties everywhere)"""
    rs = np.random.RandomState(21)
    flat = rs.random_sample((500, 3))
    flat[:, 2] = 0.375
    return {'one': np.array([[0.25, -0.5, 0.75]], dtype=np.float32),
            'two': np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]], dtype=np.float32),
            'five': (rs.random_sample((5, 3)) - 0.5).astype(np.float32),
            'copies': np.tile(np.array([0.5, 0.25, 0.125], dtype=np.float32), (3000, 1)),
            'coplanar': flat.astype(np.float32),
            'clustered': clustered_points(4000)[0],
            'lattice': lattice_points(8, 2.0 ** -4)}


def nn_queries(target_f32, n, seed=3, far_at=None):
    """n queries for a target, by index modulo 4: 0 points up to 10 box sizes outside the box (so that elements 64 and
    1024, the first of the reduction's second wave and second stride, carry a large term), 1 the target's own points
    (distance 0), 2 points inside the box, 3 in turn a corner of the box and a point with coordinates of -0.0.
    ``far_at``: that query alone is put 40 box sizes away -- the single largest distance, at a chosen index."""
    t = np.asarray(target_f32, dtype=np.float64)
    lo, hi = t.min(axis=0), t.max(axis=0)
    size = max(float((hi - lo).max()), 1.0)
    rs = np.random.RandomState(seed)
    q = lo + (hi - lo) * rs.random_sample((n, 3))
    i = np.arange(n)
    own = i % 4 == 1
    q[own] = t[(i[own] // 4) % len(t)]
    out = i % 4 == 0
    q[out] = (lo + hi) / 2 + size * rs.uniform(1.0, 10.0, (int(out.sum()), 3)) * rs.choice([-1.0, 1.0], (int(out.sum()), 3))
    for k in i[i % 4 == 3]:
        if (k // 4) % 2 == 0:
            bits = (k // 8) % 8
            q[k] = [hi[a] if (bits >> a) & 1 else lo[a] for a in range(3)]
        else:
            q[k] = [-0.0, q[k, 1], -0.0] if (k // 8) % 2 else [-0.0, -0.0, -0.0]
    if far_at is not None:
        q[far_at] = (lo + hi) / 2 + 40.0 * size * np.array([1.0, -1.0, 1.0])
    return q.astype(np.float32)


M_LIST = (1, 2, 255, 256, 257, 511, 513, 1023, 1024, 1025, 3000)       # around every multiple of the 256-point tile
REMOVE_CLOSE_INPUTS = ('uniform', 'clustered', 'lattice_h', 'lattice_2h', 'straddling', 'stacks_r0')


def remove_close_input(name, m):
    """-> (points [m, 3] float32, radius) of the named recipe at m points"""
    h = 2.0 ** -5
    if name == 'uniform':
        return uniform_points(m), 0.03
    if name == 'clustered':
        return clustered_points(m)[0], 0.02
    if name == 'stacks_r0':                      # radius 0: only exact duplicates are close, every pair of a stack ties
        return clustered_points(m)[0], 0.0
    if name == 'lattice_h':
        return lattice_points(lattice_side(m), h, m), h
    if name == 'lattice_2h':
        return lattice_points(lattice_side(m), h, m), 2.0 * h
    if name == 'straddling':
        p, _, r = straddling_points(m)
        return p, r
    raise ValueError(name)


FIXTURE_SEED = 123                       # tests/test_metrics_model.py: the leave-out rule holds for the three fixture meshes
EVEN_SEED = 9                            # ... and the even sampling at count 300 is decided


def even_lattice_mesh():
    """the exact mesh of the end-to-end even sampling: two chunks of the scan, zero-area faces at every standard place"""
    return lattice_mesh(1025, degenerate_positions(1025))
