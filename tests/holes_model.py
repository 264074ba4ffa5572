"""The numpy / Python model of DESIGN 4.8 f16 (include/p2s_hip.h: p2s_mesh_fill_holes, rules b to e), with no device: the same
float64 operations in the same association as the kernels (every product, sum and square root rounded once, no fused
multiply-add), dictionaries and loops where the device has an edge table, pointer jumping and one workgroup per loop.  The
meshes of the tests are built here too: `cup` closes everything but one loop, so the loop's numbering and positions are free."""
import itertools
import math

import numpy as np

MAX_EDGES = 128
FILLED, TOO_LONG, BLOCKED = 0, 1, 2


def edge_counts(faces):
    """{(min, max): number of faces}"""
    cnt = {}
    for f in np.asarray(faces).reshape(-1, 3).tolist():
        for e in range(3):
            a, b = f[e], f[(e + 1) % 3]
            k = (min(a, b), max(a, b))
            cnt[k] = cnt.get(k, 0) + 1
    return cnt


def boundary(faces):
    """the boundary edges a -> b as their one face traverses them, in face order"""
    cnt = edge_counts(faces)
    out = []
    for f in np.asarray(faces).reshape(-1, 3).tolist():
        for e in range(3):
            a, b = f[e], f[(e + 1) % 3]
            if cnt[(min(a, b), max(a, b))] == 1:
                out.append((a, b))
    return out


def loops(faces, n_verts):
    """rule b: the loops as vertex lists from their smallest vertex, in ascending order of it"""
    outc, inc, nxt = [0] * n_verts, [0] * n_verts, [-1] * n_verts
    for a, b in boundary(faces):
        outc[a] += 1
        inc[b] += 1
        nxt[a] = b
    simple = [outc[v] == 1 and inc[v] == 1 for v in range(n_verts)]
    found = []
    for v in range(n_verts):
        if not simple[v]:
            continue
        loop, x = [v], nxt[v]
        while x != v and simple[x] and x > v and len(loop) <= n_verts:
            loop.append(x)
            x = nxt[x]
        if x == v:
            assert len(loop) >= 3
            found.append(loop)
    return found


def area(p, i, k, j):
    """rule c: A(i, k, j) from the float64 of the corners"""
    u = [p[k][c] - p[i][c] for c in range(3)]
    w = [p[j][c] - p[i][c] for c in range(3)]
    n = (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])
    return 0.5 * math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])


def triangulate(p, forbidden=()):
    """rule c on the loop positions p [n][3] (floats): W(0, n - 1) and the split table lam (None where the hole is blocked).
    forbidden: the chords (i, j), i < j, that are edges of the mesh."""
    n = len(p)
    P = np.asarray(p, np.float64)
    W = np.zeros((n, n), np.float64)
    lam = np.zeros((n, n), np.int64)
    forbidden = set(forbidden)
    for d in range(2, n):
        for i in range(n - d):
            j = i + d
            if (i, j) in forbidden and (i, j) != (0, n - 1):
                W[i, j] = np.inf
                lam[i, j] = i + 1
                continue
            k = np.arange(i + 1, j)
            u, w = P[k] - P[i], P[j] - P[i]
            nx = u[:, 1] * w[2] - u[:, 2] * w[1]
            ny = u[:, 2] * w[0] - u[:, 0] * w[2]
            nz = u[:, 0] * w[1] - u[:, 1] * w[0]
            a = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
            cand = (W[i, k] + W[k, j]) + a
            best = int(np.argmin(cand))                 # the first minimum: the smallest k
            W[i, j] = cand[best]
            lam[i, j] = i + 1 + best if np.isfinite(cand[best]) else i + 1
    total = float(W[0, n - 1])
    return (total, lam) if math.isfinite(total) else (total, None)


def emit(lam, n):
    """rule d: the triangles (i, j, k) in the pre-order of the split tree"""
    out, stack = [], [(0, n - 1)]
    while stack:
        i, j = stack.pop()
        if j - i < 2:
            continue
        k = int(lam[i, j])
        out.append((i, j, k))
        stack.append((k, j))
        stack.append((i, k))
    return out


def all_triangulations(i, j):
    """every triangulation of the polygon i .. j as a list of triangles (i, k, j)"""
    if j - i < 2:
        return [[]]
    out = []
    for k in range(i + 1, j):
        for left in all_triangulations(i, k):
            for right in all_triangulations(k, j):
                out.append([(i, k, j)] + left + right)
    return out


def boundary_groups(faces):
    """connected groups of the boundary edges (edges that share a vertex are connected)"""
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in boundary(faces):
        parent.setdefault(a, a)
        parent.setdefault(b, b)
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return len({find(x) for x in parent})


def fill(verts, faces, max_hole_edges):
    """p2s_mesh_fill_holes: dict(faces [F', 3] int32, face_src [F'] int32, holes [H, 4] int32, hole_area [H] float64,
    report [16] int64)"""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    V, F, K = len(verts), len(faces), int(max_hole_edges)
    assert 0 <= K <= MAX_EDGES
    rep = np.zeros(16, np.int64)
    rep[0] = V | (F << 32)
    cnt = edge_counts(faces)
    P = verts.astype(np.float64)
    added, holes, areas = [], [], []
    for loop in loops(faces, V):
        n = len(loop)
        rep[2] += 1
        if n > K:
            rep[5] += 1
            holes.append((loop[0], n, -1, TOO_LONG))
            areas.append(0.0)
            continue
        forbidden = [(i, j) for i in range(n) for j in range(i + 2, n)
                     if (i, j) != (0, n - 1) and (min(loop[i], loop[j]), max(loop[i], loop[j])) in cnt]
        total, lam = triangulate(P[loop].tolist(), forbidden)
        if lam is None:
            rep[6] += 1
            holes.append((loop[0], n, -1, BLOCKED))
            areas.append(0.0)
            continue
        holes.append((loop[0], n, F + len(added), FILLED))
        areas.append(total)
        added += [(loop[i], loop[j], loop[k]) for i, j, k in emit(lam, n)]
        rep[3] += 1
        rep[10] = max(rep[10], n)
    out = np.concatenate([faces, np.asarray(added, np.int32).reshape(-1, 3)]).astype(np.int32)
    cnt_out = edge_counts(out)
    rep[1], rep[4] = len(out), len(added)
    rep[7] = sum(1 for c in cnt.values() if c == 1)
    rep[8] = sum(1 for c in cnt_out.values() if c == 1)
    rep[9] = boundary_groups(out)
    rep[11] = sum(1 for c in cnt_out.values() if c > 2)
    assert rep[11] == sum(1 for c in cnt.values() if c > 2)
    return dict(faces=out, face_src=np.concatenate([np.arange(F), np.full(len(added), -1)]).astype(np.int32),
                holes=np.asarray(holes, np.int32).reshape(-1, 4), hole_area=np.asarray(areas, np.float64), report=rep)


def fan_area(p):
    """the area of the fan from vertex 0 (what rule e of p2s_mesh_repair writes)"""
    return sum(area(p, 0, k, k + 1) for k in range(1, len(p) - 1))


# ---- the guarantees of rule f, by brute force
def vertex_fans(faces):
    """{vertex: number of fans}: the classes of the faces at a vertex that edges of exactly two faces connect"""
    faces = np.asarray(faces).reshape(-1, 3).tolist()
    cnt = edge_counts(faces)
    at = {}
    for f, tri in enumerate(faces):
        for v in tri:
            at.setdefault(v, []).append(f)
    fans = {}
    for v, fs in at.items():
        parent = {f: f for f in fs}

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x
        for f, g in itertools.combinations(fs, 2):
            shared = (set(faces[f]) & set(faces[g])) - {v}
            if any(cnt[(min(v, w), max(v, w))] == 2 for w in shared):
                parent[max(find(f), find(g))] = min(find(f), find(g))
        fans[v] = len({find(f) for f in fs})
    return fans


def check_guarantees(verts, faces, m, max_hole_edges):
    """rule f on the result m of fill(verts, faces, max_hole_edges)"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    before, after = edge_counts(faces), edge_counts(m['faces'])
    assert sum(1 for c in after.values() if c > 2) == sum(1 for c in before.values() if c > 2)
    assert all(after[k] <= max(2, before.get(k, 0)) for k in after)
    fb, fa = vertex_fans(faces), vertex_fans(m['faces'])
    assert all(fa[v] <= fb[v] for v in fb)
    for a, b in boundary(m['faces']):                       # what remains open was open
        assert before[(min(a, b), max(a, b))] == 1
    again = fill(verts, m['faces'], max_hole_edges)
    assert again['report'][3] == 0 and again['faces'].tobytes() == m['faces'].tobytes()


# ---- meshes
def cup(loop_pos, ids=None, first_id=0):
    """a mesh whose only boundary is the loop: loop vertex c has the position loop_pos[c] and the id ids[c] (default c); behind
    it a ring of n further vertices and an apex.  The boundary runs ids[0] -> ids[1] -> ...  Returns verts, faces."""
    p = np.asarray(loop_pos, np.float64).reshape(-1, 3)
    n = len(p)
    ids = list(range(n)) if ids is None else list(ids)
    assert sorted(ids) == list(range(n))
    c = p.mean(axis=0)
    verts = np.zeros((2 * n + 1, 3), np.float64)
    inner = [first_id + i for i in ids]
    outer = [first_id + n + i for i in range(n)]
    apex = first_id + 2 * n
    for i in range(n):
        verts[ids[i]] = p[i]
        verts[n + i] = c + 2.0 * (p[i] - c) + np.array([0.0, 0.0, -1.0])
    verts[2 * n] = c + np.array([0.0, 0.0, -3.0])
    faces = []
    for i in range(n):
        j = (i + 1) % n
        faces += [(inner[i], inner[j], outer[j]), (inner[i], outer[j], outer[i]), (apex, outer[i], outer[j])]
    return verts.astype(np.float32), np.asarray(faces, np.int32)


def tetra_on(verts, faces, a, b):
    """the mesh with a closed tetrahedron on the existing vertices a, b and two new ones: {a, b} becomes an edge of the mesh, and
    no boundary edge is added"""
    V = len(verts)
    x, y = V, V + 1
    extra = np.array([verts[a] + [0.3, 0.1, 2.0], verts[b] + [0.1, 0.3, 2.5]], np.float32)
    t = np.array([(a, b, x), (b, a, y), (a, x, y), (x, b, y)], np.int32)
    return np.concatenate([verts, extra]).astype(np.float32), np.concatenate([faces, t]).astype(np.int32)


def join(meshes):
    vs, fs, at = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32).reshape(-1, 3))
        fs.append(np.asarray(f, np.int32).reshape(-1, 3) + at)
        at += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def renumber(verts, faces, rng):
    """the same mesh under a random permutation of the vertex ids"""
    perm = rng.permutation(len(verts))
    v = np.zeros_like(verts)
    v[perm] = verts
    return v, perm[faces].astype(np.int32)


L_HEXAGON = [(0, 0, 0), (2, 0, 0), (2, 1, 0), (1, 1, 0), (1, 2, 0), (0, 2, 0)]      # area 3
CONVEX = [(0, 0, 0), (3, 0, 0), (5, 2, 0), (5, 4, 0), (3, 6, 0), (0, 6, 0), (-2, 4, 0), (-2, 2, 0)]      # integer, convex: all tie


def rotated(p, r):
    """the loop numbered from corner r: position c of the result is corner (c + r) mod n"""
    return [p[(c + r) % len(p)] for c in range(len(p))]


def random_loop(n, rng):
    """n float32 points near a circle, not planar"""
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = rng.uniform(0.6, 1.4, n)
    return np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-0.3, 0.3, n)], axis=1).astype(np.float32)


def sphere(nlat=12, nlon=16):
    """a closed unit sphere, outward faces"""
    verts = [(0.0, 0.0, 1.0)]
    for a in range(1, nlat):
        th = math.pi * a / nlat
        for b in range(nlon):
            ph = 2 * math.pi * b / nlon
            verts.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    verts.append((0.0, 0.0, -1.0))
    ring = lambda a, b: 1 + (a - 1) * nlon + b % nlon
    faces = []
    for b in range(nlon):
        faces.append((0, ring(1, b), ring(1, b + 1)))
        faces.append((len(verts) - 1, ring(nlat - 1, b + 1), ring(nlat - 1, b)))
    for a in range(1, nlat - 1):
        for b in range(nlon):
            faces.append((ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)))
            faces.append((ring(a, b), ring(a + 1, b + 1), ring(a, b + 1)))
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def cut(faces, around):
    """the faces without those that contain a vertex of `around`"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    return faces[~np.isin(faces, list(around)).any(axis=1)]


def octahedron():
    v = np.array([(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)
    f = np.array([(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4), (1, 0, 5), (2, 1, 5), (3, 2, 5), (0, 3, 5)], np.int32)
    return v, f


def small_cases():
    """{name: (verts, faces, max_hole_edges)}: every case of the issue that needs no long loop"""
    rng = np.random.default_rng(16)
    c = {}
    for n in (3, 4, 5):
        c['loop%d' % n] = cup(random_loop(n, rng)) + (30,)
    for r in range(6):
        c['l_hexagon_%d' % r] = cup(rotated(L_HEXAGON, r)) + (30,)
    c['convex_all_ties'] = cup(CONVEX) + (30,)
    c['collinear'] = cup([(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (3, 1, 0), (2, 1, 0), (1, 1, 0), (0, 1, 0)]) + (30,)
    c['coincident'] = cup([(0, 0, 0), (1, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 0), (0, 1, 0), (0, 0, 0)]) + (30,)
    c['all_on_a_line'] = cup([(float(i), 0, 0) for i in range(6)]) + (30,)
    # the best chord of the pentagon is an edge of the mesh already: the fill takes the next best
    p5 = [(0, 0, 0), (4, 0, 0.5), (4.5, 1, 0), (2, 1.2, 0.7), (-0.5, 1, 0)]         # not planar: one best triangulation
    v, f = cup(p5)
    free = fill(v, f, 30)['faces'][len(f):].tolist()            # loop vertex c has the id c
    used = {(min(a, b), max(a, b)) for t in free for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    chord = next(ch for ch in sorted(used) if ch[1] - ch[0] >= 2 and ch != (0, 4))
    c['best_chord_exists'] = tetra_on(v, f, *chord) + (30,)
    # two triangles whose common edge is one chord of their 4-loop; with a tetrahedron on the other chord the loop is blocked
    v = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0.5), (0, 1, 0)], np.float32)
    f = np.array([(0, 1, 2), (0, 2, 3)], np.int32)
    c['one_chord_exists'] = (v, f, 30)
    c['both_chords_exist'] = tetra_on(v, f, 1, 3) + (30,)
    # two loops that meet in one vertex: the first loop vertex of the second cup is the first of the first
    v1, f1 = cup(random_loop(5, rng))
    v2, f2 = cup(random_loop(6, rng) + np.float32(5.0))
    v, f = join([(v1, f1), (v2, f2)])
    f[f == len(v1)] = 0
    c['two_loops_meet'] = (v, f, 30)
    v, f = cup(random_loop(6, rng))
    f = f.copy()
    f[0] = f[0][[0, 2, 1]]
    c['flipped_neighbour'] = (v, f, 30)
    c['closed'] = octahedron() + (30,)
    c['no_faces'] = (np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32), 30)
    c['nothing_at_all'] = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 30)
    v, f = join([cup(random_loop(n, rng)) for n in (3, 7, 12)])
    c['a_copy'] = (v, f, 0)
    c['limit_7'] = (v, f, 7)
    c['permuted'] = renumber(*join([cup(random_loop(n, rng)) for n in (9, 4, 17, 3, 33, 31, 32)]), rng) + (32,)
    return c


def long_cases():
    """{name: (verts, faces, max_hole_edges)}: the loops around the bounds of the kernels and of the contract"""
    rng = np.random.default_rng(1995)
    c = {}
    for n in (63, 64, 65, 127, 128):
        c['loop%d' % n] = renumber(*cup(random_loop(n, rng)), rng) + (128,)
    c['loop129_left'] = cup(random_loop(129, rng)) + (128,)
    c['loop128_left_at_127'] = cup(random_loop(128, rng)) + (127,)
    return c


def many_holes(count=300, seed=2003):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(3, 41, count)
    v, f = join([cup(random_loop(int(n), rng) + np.float32(4.0 * i)) for i, n in enumerate(sizes)])
    return renumber(v, f, rng) + (30,)


def sphere_with_holes():
    """the closed sphere and the same sphere with six holes of 3 .. 60 edges -> verts, closed faces, cut faces"""
    v, f = sphere(24, 32)
    ring = lambda a, b: 1 + (a - 1) * 32 + b % 32
    g = np.delete(f, [242], axis=0)                                           # one face between rings 3 and 4: 3 edges
    g = cut(g, [ring(6, 3)])                                                  # a vertex: 6 edges
    g = cut(g, [ring(12, 10), ring(12, 11)])                                  # 8 edges
    g = cut(g, [ring(20, b) for b in range(2, 9)])
    g = cut(g, [0])                                                           # the north cap: 32 edges
    g = cut(g, [ring(10, b) for b in range(18, 24)] + [ring(11, b) for b in range(18, 24)])
    return v, f, g
