"""The numpy / Python model of DESIGN 4.8 f15 (include/p2s_hip.h: p2s_mesh_manifold, rules a to e), with no device: dictionaries
of edges, a sequential union-find over the face corners, the same float64 expression for q.  Also an independent brute-force
checker of the guarantee (rule f) and the meshes that the CPU and the GPU tests share."""
import collections

import numpy as np

import components_model as CM

MODES = (1, 2, 3)


def face_q(verts, faces):
    """q = (n.x n.x + n.y n.y) + n.z n.z per face, float64, exactly as include/p2s_hip.h writes it"""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    u, v = b - a, c - a
    nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return (nx * nx + ny * ny) + nz * nz


def edge_faces(faces):
    """(lo, hi) -> the faces that use the undirected edge, ascending"""
    table = collections.defaultdict(list)
    for i, (a, b, c) in enumerate(np.asarray(faces, np.int64).reshape(-1, 3).tolist()):
        for x, y in ((a, b), (b, c), (c, a)):
            table[(min(x, y), max(x, y))].append(i)
    return table


def manifold(verts, faces, mode):
    """dict: verts float32 [V', 3], faces int32 [F', 3], vert_src int32 [V'], face_src int32 [F'], report int64 [16]
    (report [11], the hook rounds, stays 0: not contract)"""
    p = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = p.shape[0], f.shape[0]
    if mode not in MODES:
        raise ValueError('mode')
    if not np.all(np.isfinite(p)):
        raise ValueError('non-finite vertex')
    if F and (f.min() < 0 or f.max() >= V):
        raise ValueError('face index out of range')
    if np.any((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])):
        raise ValueError('a face with a repeated index')
    report = np.zeros(16, np.int64)
    report[0] = V | (F << 32)
    edges_in = edge_faces(f)
    report[3] = sum(len(v) > 2 for v in edges_in.values())
    report[8] = sum(len(v) == 1 for v in edges_in.values())

    # b. the keepers of every edge of more than two faces; one pass
    kept = np.ones(F, bool)
    if mode & 1:
        q = face_q(p, f)
        rank = np.empty(F, np.int64)
        rank[np.lexsort((np.arange(F), -q))] = np.arange(F)          # q descending, then face id ascending
        for users in edges_in.values():
            if len(users) > 2:
                for g in sorted(users, key=lambda g: rank[g])[2:]:
                    kept[g] = False
    src = np.flatnonzero(kept)
    wf = f[src]
    F1 = wf.shape[0]

    # c. the classes of the corners
    if mode & 2:
        la, lb = [], []
        for (a, b), users in edge_faces(wf).items():
            if len(users) == 2:
                g, h = users
                for v in (a, b):
                    la.append(3 * g + wf[g].tolist().index(v))
                    lb.append(3 * h + wf[h].tolist().index(v))
        root = CM.union_find(3 * F1, la, lb)
    else:
        first = {}
        for c, v in enumerate(wf.reshape(-1).tolist()):
            first.setdefault(v, c)
        root = np.array([first[v] for v in wf.reshape(-1).tolist()], np.int64)

    # d. the output: classes ordered by (input vertex, root corner = smallest face)
    corner_v = wf.reshape(-1)
    heads = sorted({(int(corner_v[r]), int(r)) for r in root.tolist()})
    oid = {r: k for k, (_, r) in enumerate(heads)}
    vsrc = np.array([v for v, _ in heads], np.int64)
    fo = np.array([oid[r] for r in root.tolist()], np.int64).reshape(-1, 3)
    V1 = len(heads)

    # e. the report
    referenced = np.unique(corner_v).size
    per_vertex = collections.Counter(vsrc.tolist())
    edges_out = edge_faces(fo)
    report[1] = V1
    report[2] = F1
    report[4] = F - F1
    report[5] = sum(k > 1 for k in per_vertex.values())
    report[6] = V1 - referenced
    report[7] = V - referenced
    report[9] = sum(len(v) == 1 for v in edges_out.values())
    report[10] = sum(len(users) == 2 and len(edges_in[(min(vsrc[a], vsrc[b]), max(vsrc[a], vsrc[b]))]) > 2
                     for (a, b), users in edges_out.items())
    return dict(verts=p[vsrc] if V1 else np.zeros((0, 3), np.float32), faces=fo.astype(np.int32).reshape(-1, 3), vert_src=vsrc.astype(np.int32),
                face_src=src.astype(np.int32), report=report)


# ---- the checker: nothing of the model above but the edge dictionary's idea, written again ------------------------------------

def defects(faces):
    """(edges of more than two faces, vertices whose star is not connected through edges of exactly two faces): brute force"""
    f = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
    uses = collections.Counter()
    for t in f:
        for i in range(3):
            uses[frozenset((t[i], t[(i + 1) % 3]))] += 1
    star = collections.defaultdict(list)
    for i, t in enumerate(f):
        for v in t:
            star[v].append(i)
    bad_vertices = 0
    for v, fs in star.items():
        reached, todo = {fs[0]}, [fs[0]]
        while todo:
            g = todo.pop()
            for h in fs:
                if h in reached:
                    continue
                common = (set(f[g]) & set(f[h])) - {v}
                if any(uses[frozenset((v, w))] == 2 for w in common):
                    reached.add(h)
                    todo.append(h)
        bad_vertices += len(reached) < len(fs)
    return sum(c > 2 for c in uses.values()), bad_vertices


# ---- the cases of the tests ------------------------------------------------------------------------------------------------

def merge(meshes, identify=()):
    """the meshes under one index space; ``identify``: (mesh i, vertex a, mesh j, vertex b) pairs, i < j, that make vertex b of
    mesh j the same index as vertex a of mesh i (with its coordinates); the vertices left without a face stay, unreferenced"""
    vs, fs, base = [], [], [0]
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32).reshape(-1, 3))
        base.append(base[-1] + vs[-1].shape[0])
    remap = np.arange(base[-1])
    for i, a, j, b in identify:
        remap[base[j] + b] = remap[base[i] + a]
    for k, (v, f) in enumerate(meshes):
        fs.append(remap[np.asarray(f, np.int64).reshape(-1, 3) + base[k]])
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def book(pages, equal=False):
    """``pages`` faces on the spine (0, 1); with ``equal`` the first three have q = 1 exactly"""
    tips = [[0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0.5, -2]] if equal else [[0, k + 1.0, 0.25 * k] for k in range(pages)]
    v = np.array([[0, 0, 0], [1, 0, 0]] + tips[:pages], np.float32)
    return v, np.array([[0, 1, 2 + k] if k % 2 == 0 else [1, 0, 2 + k] for k in range(pages)], np.int32)


def octahedron(centre=(0.0, 0.0, 0.0)):
    """vertices 0..3 the equator, 4 the top, 5 the bottom; outward"""
    v = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) + np.asarray(centre)
    f = [[k, (k + 1) % 4, 4] for k in range(4)] + [[(k + 1) % 4, k, 5] for k in range(4)]
    return v.astype(np.float32), np.array(f, np.int32)


def cone(n, first, apex=0, height=1.0, radius=1.0):
    """a closed fan of n faces around ``apex`` over the ring of vertices first .. first + n - 1 (vertex array of first + n rows)"""
    t = np.arange(n) * (2 * np.pi / n)
    v = np.zeros((first + n, 3))
    v[first:] = np.stack([radius * np.cos(t), radius * np.sin(t), np.full(n, height)], -1)
    k = np.arange(n)
    return v.astype(np.float32), np.stack([np.full(n, apex), first + k, first + (k + 1) % n], -1).astype(np.int32)


def two_fans(seed=7):
    """a closed fan of 100 faces and one of 70 around vertex 0, the face order and the vertex ids permuted"""
    va, fa = cone(100, 1)
    vb, fb = cone(70, 101, height=-1.0, radius=0.7)
    vb[:101] = va
    return CM.join([(vb, np.concatenate([fa, fb]))], seed=seed)


def strip_with_thirds(n=300, every=7, seed=None):
    """a strip of n faces; every ``every``-th interior edge carries a third face"""
    k = np.arange(n + 2)
    v = [np.stack([k * 0.5, (k % 2) * 1.0, np.zeros(k.shape[0])], -1)]
    f = [np.stack([k[:-2], k[1:-1], k[2:]], -1)]
    nxt = n + 2
    for e in range(0, n - 1, every):                        # the edge (e + 1, e + 2) of the faces e and e + 1
        v.append(np.array([[e * 0.5 + 0.6, 0.5, 0.3 + 0.01 * e]]))
        f.append(np.array([[e + 1, e + 2, nxt]]))
        nxt += 1
    return CM.join([(np.concatenate(v), np.concatenate(f))], seed=seed)


def over_removal():
    """face 0 is rejected at the edge (0, 1) by the larger faces 1 and 2 and is a keeper at the edge (1, 2), where it displaces
    face 4: both go, and the edge (1, 2) ends with face 3 alone"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 3], [0, -2, -2], [3, 3, 3], [0.5, 0.5, 0.1]], np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4], [1, 2, 5], [2, 1, 6]], np.int32)


def soup(rng):
    """4 to 13 vertices, up to 45 distinct faces"""
    nv = int(rng.randint(4, 14))
    want = int(rng.randint(1, 46))
    seen, faces = set(), []
    for _ in range(want):
        t = rng.choice(nv, 3, replace=False)
        if frozenset(t.tolist()) not in seen:
            seen.add(frozenset(t.tolist()))
            faces.append(t)
    return rng.normal(size=(nv, 3)).astype(np.float32), np.array(faces, np.int32)


def small_cases():
    """name -> (verts, faces): the smallest shapes at which the kernels can go wrong"""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    ta, tb = CM.tetra(1.0), (CM.tetra(1.0)[0] + np.float32(3.0), CM.tetra(1.0)[1])
    oa, ob = octahedron(), octahedron((0.5, 0.5, 3.0))
    b3 = book(3)
    pad = np.array([[9, 9, 9]], np.float32)
    cases = {
        'empty': (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
        'vertices_only': (tri, np.zeros((0, 3), np.int32)),
        'one_face': (tri, np.array([[0, 1, 2]], np.int32)),
        'book3': b3,
        'book4': book(4),
        'tetra': ta,
        'tetras_sharing_a_vertex': merge([ta, tb], [(0, 0, 1, 0)]),
        'tetras_sharing_an_edge': merge([ta, tb], [(0, 0, 1, 0), (0, 1, 1, 1)]),
        # tetrahedra that share two edges share the face between them; octahedra share the equator chain 0 - 1 - 2 and no face
        'octahedra_sharing_two_edges': merge([oa, ob], [(0, 0, 1, 0), (0, 1, 1, 1), (0, 2, 1, 2)]),
        'two_fans': two_fans(),
        'strip_with_thirds': strip_with_thirds(),
        'strip_with_thirds_permuted': strip_with_thirds(seed=5),
        'duplicate_faces': (tri, np.array([[0, 1, 2], [0, 1, 2]], np.int32)),
        'duplicate_faces_on_an_edge': (np.concatenate([tri, [[0, 0, 2]]]).astype(np.float32), np.array([[0, 1, 2], [1, 0, 3], [2, 1, 0]], np.int32)),
        'unreferenced_vertices': (np.concatenate([pad, b3[0][:3], pad, pad, b3[0][3:], pad]),
                                  np.array([[1, 2, 3], [2, 1, 6], [1, 2, 7]], np.int32)),
        'equal_q': book(3, equal=True),
        'equal_q_four': book(4, equal=True),
        'over_removal': over_removal(),
    }
    rng = np.random.RandomState(2024)
    for k in range(200):
        cases['soup%03d' % k] = soup(rng)
    return cases


def two_sheets():
    """two square sheets 0.02 apart, of 24 x 24 and 29 x 29 quads, the second turned by 0.5 rad in its plane: a clustering grid
    coarser than the gap merges them into one sheet with edges of more than two faces (94 of them at resolution 12)"""
    def sheet(n, z, angle, tilt):
        g = np.arange(n + 1) / n
        x, y = np.meshgrid(g, g, indexing='ij')
        c, s = np.cos(angle), np.sin(angle)
        v = np.stack([0.5 + c * (x - 0.5) - s * (y - 0.5), 0.5 + s * (x - 0.5) + c * (y - 0.5), z + tilt * x], -1).reshape(-1, 3)
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        a, b, d, e = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
        return v.astype(np.float32), np.concatenate([np.stack([a, b, d], -1).reshape(-1, 3), np.stack([a, d, e], -1).reshape(-1, 3)])
    return CM.join([sheet(24, 0.0, 0.0, 0.0), sheet(29, 0.02, 0.5, 0.01)])


def big_case(seed=13):
    """39,600 faces: three tori of 100 x 66 quads; the second shares the first one's ring i = 0 (66 vertices, 66 edges that then
    carry four faces), the third shares one vertex with the first and a chain of 5 edges with the second; the face order and
    the vertex ids permuted"""
    nu, nv = 100, 66
    t = [CM.torus(nu, nv), CM.torus(nu, nv, centre=(0.2, 0.0, 0.3)), CM.torus(nu, nv, centre=(-0.3, 0.4, 0.0))]
    identify = [(0, j, 1, j) for j in range(nv)]
    identify += [(0, 50 * nv + 7, 2, 3 * nv + 9)]
    identify += [(1, 40 * nv + j, 2, 70 * nv + j) for j in range(10, 16)]
    return CM.join([merge(t, identify)], seed=seed)
