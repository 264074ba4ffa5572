"""CPU model of p2s_mesh_check (include/p2s_hip.h): every pair of faces classified by brute force in numpy float64 with the
kernel's operations in the kernel's association (dot3 = (x + y) + z, cross3, orient3 = ((b - a) x (c - a)) . (d - a)), and the
fan walk around every vertex run serially.  Also the three meshes the tests are built on."""
import numpy as np

DEGENERATE_REL = 2.0 ** -90
DISJOINT, INTERSECTING, COPLANAR, TOUCHING, DUPLICATE = 0, 1, 2, 3, 4
FACE_INTERSECTING, FACE_COPLANAR, FACE_TOUCHING, FACE_DEGENERATE = 1, 2, 4, 8
REPORT_KEYS = ('faces_tested', 'faces_degenerate', 'candidates', 'intersecting', 'coplanar', 'touching', 'duplicate',
               'faces_flagged', 'pairs_inside_component', 'pairs_across_components', 'nonmanifold_vertices', 'pairs_stored')


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


def bounds(scale):
    """the filter bounds of a mesh whose largest |coordinate| is ``scale``: (3D, 2D)"""
    s = np.float64(scale)
    return ((s * s) * s) * 2.0 ** -43, (s * s) * 2.0 ** -47


def _drop_axis(T):
    """T [P, 3, 3] -> the two kept axes [P, 2] after dropping the axis of the largest |n| (the first among equals)"""
    n = np.abs(cross3(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]))
    ax = np.zeros(len(T), np.int64)
    ax[n[:, 1] > n[:, 0]] = 1
    big = np.maximum(n[:, 0], n[:, 1])
    ax[n[:, 2] > big] = 2
    keep = np.array([[1, 2], [0, 2], [0, 1]])
    return keep[ax]


def _project(T, keep):
    r = np.arange(len(T))[:, None, None]
    return T[r, np.arange(T.shape[1])[None, :, None], keep[:, None, :]]


def _seg_in_plane(p, q, T, eps2):
    """an edge p-q in the plane of T: 0 = strictly apart in 2D, 1 = possibly meeting"""
    keep = _drop_axis(T)
    T2 = _project(T, keep)
    pq = _project(np.stack([p, q], 1), keep)
    o = sgn(orient2(T2[:, 0], T2[:, 1], T2[:, 2]), eps2)
    apart = np.zeros(len(T), bool)
    r = []
    for k in range(3):
        x, y = T2[:, k], T2[:, (k + 1) % 3]
        apart |= (o * sgn(orient2(x, y, pq[:, 0]), eps2) < 0) & (o * sgn(orient2(x, y, pq[:, 1]), eps2) < 0)
        r.append(sgn(orient2(pq[:, 0], pq[:, 1], T2[:, k]), eps2))
    apart |= (r[0] != 0) & (r[0] == r[1]) & (r[1] == r[2])
    return np.where((o != 0) & apart, 0, 1)


def _edge_test(p, q, T, sp, sq, eps3, eps2):
    """0 = no, 1 = possible, 2 = strict: the edge p-q pierces the interior of T"""
    out = np.zeros(len(T), np.int64)
    live = ~(sp * sq > 0)
    inpl = live & (sp == 0) & (sq == 0)
    if inpl.any():
        out[inpl] = _seg_in_plane(p[inpl], q[inpl], T[inpl], eps2)
    rest = live & ~inpl
    if rest.any():
        P, Q, TT = p[rest], q[rest], T[rest]
        v = np.stack([sgn(orient3(P, Q, TT[:, k], TT[:, (k + 1) % 3]), eps3) for k in range(3)], 1)
        pos, neg, zero = (v > 0).any(1), (v < 0).any(1), (v == 0).any(1)
        strict = (sp[rest] * sq[rest] < 0) & ~zero
        out[rest] = np.where(pos & neg, 0, np.where(strict, 2, 1))
    return out


def _coplanar(A, B, shared, eps2):
    """two triangles in one plane: COPLANAR when no edge line of either has the other triangle on its outer closed side; a
    pair with a shared index that does not overlap meets in its shared vertices only: DISJOINT; without one it is DISJOINT
    when some edge line has the other triangle strictly outside, else TOUCHING"""
    keep = _drop_axis(A)
    A2, B2 = _project(A, keep), _project(B, keep)
    oA = sgn(orient2(A2[:, 0], A2[:, 1], A2[:, 2]), eps2)
    oB = sgn(orient2(B2[:, 0], B2[:, 1], B2[:, 2]), eps2)
    sep = np.zeros(len(A), bool)
    strict = np.zeros(len(A), bool)
    for P, Q, o in ((A2, B2, oA), (B2, A2, oB)):
        for e in range(3):
            x, y = P[:, e], P[:, (e + 1) % 3]
            s = np.stack([o * sgn(orient2(x, y, Q[:, j]), eps2) for j in range(3)], 1)
            sep |= (s <= 0).all(1)
            strict |= (s < 0).all(1)
    out = np.where(~sep, COPLANAR, np.where(strict | shared, DISJOINT, TOUCHING))
    return np.where((oA == 0) | (oB == 0), TOUCHING, out)


def classify(A, ia, B, ib, scale):
    """A, B [P, 3, 3] float64 triangles of non-degenerate faces, ia, ib [P, 3] their vertex indices -> class [P]"""
    eps3, eps2 = bounds(scale)
    P = len(A)
    out = np.zeros(P, np.int64)
    eq = ia[:, :, None] == ib[:, None, :]
    sa, sb = eq.any(2), eq.any(1)
    ns = sa.sum(1)
    out[ns == 3] = DUPLICATE
    box = ((A.min(1) <= B.max(1)) & (B.min(1) <= A.max(1))).all(1)
    todo = np.nonzero((ns < 3) & box)[0]
    if len(todo) == 0:
        return out
    A, B, sa, sb, ns = A[todo], B[todo], sa[todo], sb[todo], ns[todo]
    sB = np.stack([np.where(sb[:, j], 0, sgn(orient3(A[:, 0], A[:, 1], A[:, 2], B[:, j]), eps3)) for j in range(3)], 1)
    sA = np.stack([np.where(sa[:, i], 0, sgn(orient3(B[:, 0], B[:, 1], B[:, 2], A[:, i]), eps3)) for i in range(3)], 1)
    res = np.zeros(len(todo), np.int64)
    flat = (sB == 0).all(1) & (sA == 0).all(1)
    if flat.any():
        res[flat] = _coplanar(A[flat], B[flat], ns[flat] > 0, eps2)

    def one_sided(s, shared):
        return ((s > 0) | shared).all(1) | ((s < 0) | shared).all(1)
    go = np.nonzero(~flat & (ns < 2) & ~one_sided(sB, sb) & ~one_sided(sA, sa))[0]
    if len(go):
        best = np.zeros(len(go), np.int64)
        for P_, sP, shP, T in ((B, sB, sb, A), (A, sA, sa, B)):
            for e in range(3):
                e1 = (e + 1) % 3
                free = np.nonzero(~shP[go, e] & ~shP[go, e1])[0]
                if len(free):
                    k = go[free]
                    best[free] = np.maximum(best[free], _edge_test(P_[k, e], P_[k, e1], T[k], sP[k, e], sP[k, e1], eps3, eps2))
        res[go] = np.where(best == 2, INTERSECTING, np.where(best == 1, TOUCHING, DISJOINT))
    out[todo] = res
    return out


def degenerate(tri):
    ab, ac = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = cross3(ab, ac)
    return ~(dot3(n, n) > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)))


def nonmanifold_vertices(faces, n_verts):
    """flag [V]: the faces at the vertex are not one fan.  Faces are neighbours across an undirected edge that exactly two
    faces use; the walk starts at the vertex's smallest face and rotates both ways."""
    f = np.asarray(faces, np.int64)
    edge = {}
    for i, (a, b, c) in enumerate(f.tolist()):
        for x, y in ((a, b), (b, c), (c, a)):
            edge.setdefault((min(x, y), max(x, y)), []).append(i)
    deg = np.zeros(n_verts, np.int64)
    first = np.full(n_verts, -1, np.int64)
    for i, t in enumerate(f.tolist()):
        for j in range(3):
            if t[j] in t[:j]:
                continue
            deg[t[j]] += 1
            if first[t[j]] < 0:
                first[t[j]] = i
    flag = np.zeros(n_verts, np.uint8)
    for v in range(n_verts):
        if deg[v] == 0:
            continue
        f0 = int(first[v])
        t = f[f0].tolist()
        j = t.index(v)
        reached, closed = 1, False
        for w in (t[(j + 1) % 3], t[(j + 2) % 3]):
            cur = f0
            while reached < deg[v]:
                fs = edge[(min(v, w), max(v, w))]
                if len(fs) != 2:
                    break
                g = fs[0] + fs[1] - cur
                if g == cur:
                    break
                if g == f0:
                    closed = True
                    break
                reached += 1
                w = int(f[g].sum()) - v - w
                cur = g
            if closed:
                break
        flag[v] = 1 if reached < deg[v] else 0
    return flag


def components(faces, n_verts):
    """the label (smallest face id) of every face's component on a closed mesh (every edge once in each direction), else None"""
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    key = np.minimum(a, b) * n_verts + np.maximum(a, b)
    uk, inv = np.unique(key, return_inverse=True)
    fwd = np.bincount(inv[a < b], minlength=len(uk))
    bwd = np.bincount(inv[~(a < b)], minlength=len(uk))
    if not ((fwd == 1) & (bwd == 1)).all():
        return None
    face = np.tile(np.arange(len(f)), 3)
    order = np.argsort(key, kind='stable')
    adj = np.empty((len(f), 3), np.int64)
    slot = np.repeat(np.arange(3), len(f))
    p0, p1 = order[0::2], order[1::2]
    adj[face[p0], slot[p0]] = face[p1]
    adj[face[p1], slot[p1]] = face[p0]
    lab = np.arange(len(f))
    while True:
        new = np.minimum(lab, lab[adj].min(1))
        new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


def check(verts, faces, block=1 << 20):
    """-> dict: report (REPORT_KEYS; candidates = every pair of tested faces), pairs [n, 2], classes [n], face_flags [F],
    vert_flags [V]"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    F = len(f)
    tri = v[f]
    scale = float(np.abs(v).max())
    deg = degenerate(tri)
    ok = np.nonzero(~deg)[0]
    lo, hi = tri.min(1), tri.max(1)
    pairs, classes = [], []
    n_dup = 0
    for i in ok.tolist():
        g = ok[ok > i]
        for s in range(0, len(g), block):
            gg = g[s:s + block]
            gg = gg[((lo[i] <= hi[gg]) & (lo[gg] <= hi[i])).all(1)]          # what classify rejects first
            if len(gg) == 0:
                continue
            c = classify(np.broadcast_to(tri[i], (len(gg), 3, 3)), np.broadcast_to(f[i], (len(gg), 3)), tri[gg], f[gg], scale)
            n_dup += int((c == DUPLICATE).sum())
            keep = (c >= INTERSECTING) & (c <= TOUCHING)
            pairs.append(np.stack([np.full(keep.sum(), i, np.int64), gg[keep]], 1))
            classes.append(c[keep])
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    classes = np.concatenate(classes) if classes else np.zeros((0,), np.int64)
    fflag = np.where(deg, FACE_DEGENERATE, 0).astype(np.uint8)
    for cls, bit in ((INTERSECTING, FACE_INTERSECTING), (COPLANAR, FACE_COPLANAR), (TOUCHING, FACE_TOUCHING)):
        fflag[np.unique(pairs[classes == cls])] |= bit
    vflag = nonmanifold_vertices(f, len(v))
    comp = components(f, len(v))
    hard = pairs[(classes == INTERSECTING) | (classes == COPLANAR)]
    inside = int((comp[hard[:, 0]] == comp[hard[:, 1]]).sum()) if comp is not None else -1
    n_ok = len(ok)
    rep = dict(faces_tested=n_ok, faces_degenerate=int(deg.sum()), candidates=n_ok * (n_ok - 1) // 2,
               intersecting=int((classes == INTERSECTING).sum()), coplanar=int((classes == COPLANAR).sum()),
               touching=int((classes == TOUCHING).sum()), duplicate=n_dup,
               faces_flagged=int(((fflag & (FACE_INTERSECTING | FACE_COPLANAR)) != 0).sum()), pairs_inside_component=inside,
               pairs_across_components=len(hard) - inside if comp is not None else -1,
               nonmanifold_vertices=int(vflag.sum()), pairs_stored=len(pairs))
    return dict(report=rep, pairs=pairs.astype(np.int32), classes=classes.astype(np.uint8), face_flags=fflag, vert_flags=vflag)


def verdict(report, closed=True):
    """the verdict column of check_report.csv"""
    if report['intersecting'] + report['coplanar'] > 0:
        return 'self-intersecting'
    return 'non-manifold' if report['nonmanifold_vertices'] > 0 else 'embedded'


# ---------------------------------------------------------------------------------------------
# meshes of the tests
# ---------------------------------------------------------------------------------------------
def ribbon_prism(n=24, h=0.25, half_width=0.09):
    """a ribbon of width 2 half_width along the curve (t^2 - 1, t (t^2 - 1)), t in [-1.3, 1.3], which crosses itself once at
    the origin, extruded from z = 0 to z = h: one closed, consistently oriented component of positive volume whose walls
    pass through each other and whose caps overlap in their planes"""
    t = np.linspace(-1.3, 1.3, n + 1)
    p = np.stack([t * t - 1.0, t * (t * t - 1.0)], 1)
    d = np.stack([2.0 * t, 3.0 * t * t - 1.0], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    nrm = np.stack([-d[:, 1], d[:, 0]], 1)
    L, R = p + half_width * nrm, p - half_width * nrm
    m = n + 1
    v = np.concatenate([np.c_[L, np.zeros(m)], np.c_[R, np.zeros(m)], np.c_[L, np.full(m, h)], np.c_[R, np.full(m, h)]]).astype(np.float32)
    l0, r0, l1, r1 = 0, m, 2 * m, 3 * m
    f = []

    def quad(a, b, c, d_):
        f.extend([(a, b, c), (a, c, d_)])
    for i in range(n):
        quad(l1 + i, r1 + i, r1 + i + 1, l1 + i + 1)           # top
        quad(l0 + i, l0 + i + 1, r0 + i + 1, r0 + i)           # bottom
        quad(l0 + i, l1 + i, l1 + i + 1, l0 + i + 1)           # left wall
        quad(r0 + i, r0 + i + 1, r1 + i + 1, r1 + i)           # right wall
    quad(l0, r0, r1, l1)                                       # the two ends
    quad(l0 + n, l1 + n, r1 + n, r0 + n)
    f = np.array(f, np.int32)
    vd = v.astype(np.float64)
    if dot3(vd[f[:, 0]], cross3(vd[f[:, 1]], vd[f[:, 2]])).sum() < 0:
        f = f[:, [0, 2, 1]]
    return v, f


def pierced_grid(k=24):
    """the unit square z = 0 as k x k cells of two triangles each, and one large triangle through it: it crosses the square
    along a short segment near one corner, while its centroid lies far outside the square"""
    g = np.arange(k + 1, dtype=np.float64) / k
    v = [[x, y, 0.0] for x in g for y in g]
    f = []
    for i in range(k):
        for j in range(k):
            a, b, c, d = i * (k + 1) + j, (i + 1) * (k + 1) + j, (i + 1) * (k + 1) + j + 1, i * (k + 1) + j + 1
            f += [(a, b, c), (a, c, d)]
    n = len(v)
    v += [[0.07, 0.03, -0.05], [0.11, 0.21, -0.05], [6.0, 5.0, 9.0]]
    f.append((n, n + 1, n + 2))
    return np.array(v, np.float32), np.array(f, np.int32)


def bowtie():
    """two tetrahedra welded at one vertex (index 0)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2], [0, 4, 5], [0, 6, 4], [4, 6, 5], [0, 5, 6]], np.int32)
    return v, f


# the constructions with known answers
T0 = [[0, 0, 0], [2, 0, 0], [0, 2, 0]]


def _two(a, b):
    """two triangles without a common vertex"""
    return np.array(a + b, np.float32), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def crossing():
    return _two(T0, [[0.5, 0.5, -1], [0.5, 0.5, 1], [3, 3, 0.5]])


def apart():
    return _two(T0, [[0.5, 0.5, 2], [0.5, 0.5, 4], [3, 3, 3.5]])


def shared_vertex_pierce():
    """the edge opposite the shared vertex 0 of the second face passes through the first"""
    v = np.array(T0 + [[0.5, 0.5, -1], [0.6, 0.7, 1]], np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 4]], np.int32)


def adjacent():
    v = np.array(T0 + [[1.5, 1.5, 1]], np.float32)
    return v, np.array([[0, 1, 2], [2, 1, 3]], np.int32)


def fold():
    """two faces on one edge, in one plane, on the same side of it"""
    v = np.array(T0 + [[0.5, 0.25, 0]], np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3]], np.int32)


def coplanar_overlap():
    return _two(T0, [[0.5, 0.5, 0], [3, 0.5, 0], [0.5, 3, 0]])


def coplanar_apart():
    return _two(T0, [[3, 3, 0], [5, 3, 0], [3, 5, 0]])


def vertex_on_face():
    return _two(T0, [[0.5, 0.5, 0], [0.5, 0.5, 1], [1, 1, 2]])


# queries inside one branch of ribbon_prism() next to the wall of the other, where the two branches cross: picked by running
# the two models (the nearest feature belongs to the other branch's wall, whose pseudonormal points at the query)
RIBBON_QUERIES = np.array([
    (0.0944, -0.0778, 0.1651), (0.1180, -0.0438, 0.0322), (0.0901, 0.0574, 0.2008), (0.0621, -0.1275, 0.1775),
    (0.0590, -0.0978, 0.0681), (-0.0775, -0.0831, 0.0382), (0.0277, -0.1299, 0.2192), (-0.0890, -0.0743, 0.1171),
    (0.0631, -0.0884, 0.0877), (-0.0534, 0.1203, 0.2046), (0.0781, -0.0975, 0.1341), (0.0709, 0.1013, 0.1980),
    (-0.1236, -0.0670, 0.0445), (-0.1055, 0.1059, 0.1355), (-0.1007, -0.0496, 0.1068), (-0.1167, -0.0939, 0.1474),
    (0.0782, -0.0599, 0.0908), (-0.1191, 0.0780, 0.0572), (0.0217, -0.1200, 0.0358), (0.1032, 0.0818, 0.1333),
    (0.0848, -0.0781, 0.0706), (-0.1121, -0.1207, 0.0924), (-0.0873, 0.0589, 0.0965), (-0.1296, -0.0602, 0.0845)], np.float32)
