"""CPU model of the mesh repair and the normalisation (include/p2s_hip.h: p2s_mesh_repair, p2s_mesh_normalize;
points2surf_amd/csrc/p2s_meshrepair.inl; the shared kernels and build_edges: p2s_meshdist.hip): a serial restatement in plain Python / numpy -- a dict of edges, union-find with
parity, loop walking.  Everything but the volumes is integer work, so it has one right answer; the float64 volume sums
repeat the order of the device's kernels (p2s_md_volume_kernel, p2s_md_comp_volume_kernel: 1024 lanes each adding the
faces f = lane, lane + 1024, ... in turn, an xor butterfly over the 64 lanes of a wave, the 16 waves added in order)."""
import numpy as np

REPORT_KEYS = ('verts_in', 'faces_in', 'verts_out', 'faces_out', 'verts_welded', 'faces_collapsed', 'faces_duplicate',
               'faces_degenerate', 'faces_flipped', 'components', 'components_unorientable', 'components_inverted',
               'holes_filled', 'faces_added', 'holes_left', 'boundary_edges_left', 'nonmanifold_edges', 'watertight',
               'winding_consistent', 'is_volume')
DEGENERATE_REL = 2.0 ** -90


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def volume6(verts, faces, mask=None):
    """six times the signed volume of the faces (of those under ``mask``) in the device's order"""
    P = verts.astype(np.float64)[faces]
    term = _dot3(P[:, 0], _cross3(P[:, 1], P[:, 2]))
    if mask is not None:
        term = np.where(mask, term, 0.0)          # a skipped face and an added +0.0 leave the same sum
    n = len(term)
    rows = max(1, -(-n // 1024))
    t = np.zeros(rows * 1024)
    t[:n] = term
    t = t.reshape(rows, 1024)
    sm = np.zeros(1024)
    for r in range(rows):
        sm = sm + t[r]
    s = sm.reshape(16, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ d]
    total = 0.0
    for w in range(16):
        total = total + s[w, 0]
    return float(total)


def _edges(faces):
    """undirected edge -> list of (face, 0 low -> high / 1 high -> low)"""
    table = {}
    for f, (a, b, c) in enumerate(faces):
        for u, v in ((a, b), (b, c), (c, a)):
            table.setdefault((min(u, v), max(u, v)), []).append((f, 0 if u < v else 1))
    return table


class _Parity:
    """union-find; par[x] = x flipped relative to its root"""

    def __init__(self, n):
        self.parent = list(range(n))
        self.par = [0] * n

    def find(self, x):
        path = []
        while self.parent[x] != x:
            path.append(x)
            x = self.parent[x]
        acc = 0
        for y in reversed(path):
            acc ^= self.par[y]
            self.par[y] = acc
            self.parent[y] = x
        return x

    def parity(self, x):
        self.find(x)
        return self.par[x]

    def union(self, f, g, p):
        rf, rg = self.find(f), self.find(g)
        if rf == rg:
            return
        q = self.par[f] ^ self.par[g] ^ p
        hi, lo = max(rf, rg), min(rf, rg)
        self.parent[hi] = lo
        self.par[hi] = q


def check_input(verts, faces, max_hole_edges=4):
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces).astype(np.int64).reshape(-1, 3)
    if not 0 <= int(max_hole_edges) <= 64:
        raise ValueError('max_hole_edges must be in 0..64')
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError('face index out of range')
    if not np.isfinite(verts).all():
        raise ValueError('non-finite vertex')
    return verts, faces


def repair(verts, faces, max_hole_edges=4):
    """-> verts [V', 3] float32, faces [F', 3] int32, face_src [F'] int32, report dict (REPORT_KEYS)"""
    verts, faces = check_input(verts, faces, max_hole_edges)
    K = int(max_hole_edges)
    V, F = len(verts), len(faces)
    rep = dict.fromkeys(REPORT_KEYS, 0)
    rep['verts_in'], rep['faces_in'] = V, F

    def done(v, f, src):
        rep['verts_out'], rep['faces_out'] = len(v), len(f)
        return (np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3),
                np.ascontiguousarray(src, np.int32), rep)

    if F == 0:
        rep['watertight'] = rep['winding_consistent'] = 1
        return done(verts[:0], faces[:0], [])

    # b. weld: equal coordinates (-0.0 as +0.0) -> the smallest index
    bits = np.where(verts == 0, np.float32(0), verts).view(np.uint32)
    first = {}
    weld = np.empty(V, np.int64)
    for i, key in enumerate(map(tuple, bits.tolist())):
        weld[i] = first.setdefault(key, i)
    rep['verts_welded'] = int((weld != np.arange(V)).sum())

    # c. collapsed and duplicate faces
    wf, src, seen = [], [], {}
    for f, (a, b, c) in enumerate(weld[faces].tolist()):
        if a == b or b == c or c == a:
            rep['faces_collapsed'] += 1
            continue
        key = tuple(sorted((a, b, c)))
        if key in seen:
            rep['faces_duplicate'] += 1
            continue
        seen[key] = f
        wf.append([a, b, c])
        src.append(f)
    F0 = len(wf)
    if F0 == 0:
        rep['watertight'] = rep['winding_consistent'] = 1
        return done(verts[:0], faces[:0], [])
    P = verts.astype(np.float64)[np.array(wf)]
    ab, ac = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = _cross3(ab, ac)
    rep['faces_degenerate'] = int((~(_dot3(n, n) > DEGENERATE_REL * (_dot3(ab, ab) * _dot3(ac, ac)))).sum())

    # d. orient
    table = _edges(wf)
    uf = _Parity(F0)
    pairs = []
    for users in table.values():
        if len(users) == 2:
            (f, df), (g, dg) = users
            pairs.append((f, g, 0 if df != dg else 1))
    for f, g, p in pairs:
        uf.union(f, g, p)
    bad = set()
    for f, g, p in pairs:
        if uf.parity(f) ^ uf.parity(g) != p:
            bad.add(uf.find(f))
    rep['components_unorientable'] = len(bad)
    unor = [uf.find(f) in bad for f in range(F0)]
    for f in range(F0):                           # the root is the smallest id of its component and keeps its winding
        if not unor[f] and uf.parity(f):
            wf[f] = [wf[f][0], wf[f][2], wf[f][1]]
            rep['faces_flipped'] += 1

    # e. holes
    table = _edges(wf)
    outc, inc, nxt, blocked = {}, {}, {}, set()
    for (lo, hi), users in table.items():
        if len(users) != 1:
            continue
        f, d = users[0]
        a, b = (lo, hi) if d == 0 else (hi, lo)
        outc[a] = outc.get(a, 0) + 1
        inc[b] = inc.get(b, 0) + 1
        nxt[a] = b
        if unor[f]:
            blocked.update((a, b))

    def simple(v):
        return outc.get(v, 0) == 1 and inc.get(v, 0) == 1 and v not in blocked

    for v in sorted(outc):
        if not simple(v):
            continue
        loop, x, ok = [v], nxt[v], True
        while x != v:
            if len(loop) >= K or x < v or not simple(x):
                ok = False
                break
            loop.append(x)
            x = nxt[x]
        if not ok or not 3 <= len(loop) <= K:
            continue
        rep['holes_filled'] += 1
        for k in range(1, len(loop) - 1):
            wf.append([loop[0], loop[k + 1], loop[k]])
            src.append(-1)
            rep['faces_added'] += 1
    F1 = len(wf)

    # f. components again, inversion
    table = _edges(wf)
    uf = _Parity(F1)
    open_faces, bverts = set(), _Parity(V)
    on_boundary = set()
    for (lo, hi), users in table.items():
        if len(users) == 1:
            rep['boundary_edges_left'] += 1
            open_faces.add(users[0][0])
            bverts.union(lo, hi, 0)
            on_boundary.update((lo, hi))
        elif len(users) == 2:
            uf.union(users[0][0], users[1][0], 0)
            if users[0][1] == users[1][1]:
                rep['winding_consistent'] += 1    # counted here, turned into the flag below
        else:
            rep['nonmanifold_edges'] += 1
    rep['holes_left'] = len({bverts.find(v) for v in on_boundary})
    comp = np.array([uf.find(f) for f in range(F1)])
    roots = sorted(set(comp.tolist()))
    rep['components'] = len(roots)
    open_roots = {int(comp[f]) for f in open_faces}
    wfa = np.array(wf, dtype=np.int64)
    for r in roots:
        if r in open_roots:
            continue
        if volume6(verts, wfa, comp == r) < 0.0:
            rep['components_inverted'] += 1
            wfa[comp == r] = wfa[comp == r][:, [0, 2, 1]]
    rep['watertight'] = int(rep['boundary_edges_left'] == 0 and rep['nonmanifold_edges'] == 0)
    rep['winding_consistent'] = int(rep['winding_consistent'] == 0)
    rep['is_volume'] = int(bool(rep['watertight'] and rep['winding_consistent'] and volume6(verts, wfa) > 0.0))

    # g. compaction
    used = np.zeros(V, bool)
    used[wfa.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return done(verts[used], new[wfa], src)


def normalize(verts):
    """float32 [V, 3]; ValueError for a non-finite vertex or none at all, ZeroDivisionError for a zero extent"""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    if len(verts) < 1 or not np.isfinite(verts).all():
        raise ValueError('normalize needs finite vertices')
    lo, hi = verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64)
    if not ((hi - lo) > 0.0).all():
        raise ZeroDivisionError('the bounding box has a zero extent on an axis')
    c = (lo + hi) / 2.0
    s = 1.0 / (hi - lo).max()
    return ((verts.astype(np.float64) - c) * s).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# meshes of the tests
# ---------------------------------------------------------------------------------------------
def cube(lo=0.0, hi=1.0):
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                  [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f                                   # outward


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)      # outward


def icosahedron():
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p],
                  [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]], np.float32)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
                  [8, 6, 7], [9, 8, 1]], np.int32)
    return v, f


def sphere(min_faces):
    """an icosahedron subdivided until it has at least ``min_faces`` faces, cut to exactly that many when it has more
    (the cut leaves one large hole, or none)"""
    v, f = icosahedron()
    v = v.astype(np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = f.astype(np.int64)
    while len(f) < min_faces:
        mid = {}
        vs = list(v)

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = (vs[a] + vs[b]) / 2.0
                vs.append(p / np.linalg.norm(p))
                mid[k] = len(vs) - 1
            return mid[k]
        nf = []
        for a, b, c in f.tolist():
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(vs), np.array(nf, np.int64)
    return v.astype(np.float32), f[:min_faces].astype(np.int32)


def moebius(n=8):
    """a strip of 2 n triangles with a half twist"""
    v = []
    for i in range(n):
        t = 2.0 * np.pi * i / n
        for s in (-0.3, 0.3):
            r = 1.0 + s * np.cos(t / 2.0)
            v.append([r * np.cos(t), r * np.sin(t), s * np.sin(t / 2.0)])
    f = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        if i + 1 < n:
            c, d = 2 * i + 2, 2 * i + 3
        else:
            c, d = 1, 0                           # the twist
        f += [[a, c, b], [b, c, d]]
    return np.array(v, np.float32), np.array(f, np.int32)


def soup(verts, faces, seed, flip_fraction=1.0 / 3.0, invert=None, n_duplicate=100, n_collapsed=100):
    """every face its own three vertices, a seeded ``flip_fraction`` of the faces flipped, the faces ``invert`` (a mask)
    turned inside out before that, then ``n_duplicate`` duplicate faces in assorted rotations and windings and
    ``n_collapsed`` collapsed faces appended.  -> verts, faces, flipped mask [F] (of the F original faces)"""
    rng = np.random.RandomState(seed)
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    F = len(faces)
    fl = rng.rand(F) < flip_fraction
    if invert is not None:
        fl = fl ^ np.asarray(invert, bool)
    g = np.where(fl[:, None], faces[:, [0, 2, 1]], faces)
    sv = verts[g.reshape(-1)]
    sf = np.arange(3 * F).reshape(F, 3)
    extra_v, extra_f = [], []
    base = 3 * F
    perms = [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]]
    for j in range(n_duplicate):
        f = int(rng.randint(F))
        extra_v.append(verts[faces[f][perms[j % 6]]])
        extra_f.append([base, base + 1, base + 2])
        base += 3
    for j in range(n_collapsed):
        f = int(rng.randint(F))
        a, b = verts[faces[f][0]], verts[faces[f][1]]
        extra_v.append(np.stack([a, b, a] if j % 2 else [a, a, b]))
        extra_f.append([base, base + 1, base + 2])
        base += 3
    if extra_v:
        sv = np.concatenate([sv] + extra_v)
        sf = np.concatenate([sf, np.array(extra_f)])
    return sv.astype(np.float32), sf.astype(np.int32), fl
