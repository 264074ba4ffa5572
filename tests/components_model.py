"""The numpy model of DESIGN 4.8 f14 (include/p2s_hip.h: p2s_mesh_components, p2s_mesh_submesh, p2s_prepare_clusters), with no
device: a plain union-find over faces and vertices, a pair test over a cell grid for the clusters, math.fsum of the per-face
terms.  Also the meshes and clouds that the CPU and the GPU tests share."""
import math

import numpy as np


# ---- union-find ------------------------------------------------------------------------------------------------------------

def union_find(n, a, b):
    """the smallest member of every class of 0 .. n - 1 under the links a[k] -- b[k]"""
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(x) for x in range(n)], np.int64)


# ---- meshes ----------------------------------------------------------------------------------------------------------------

def face_terms(verts, faces):
    """the area and volume terms of every face, float64, exactly as include/p2s_hip.h writes them"""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    u, v = b - a, c - a
    nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    vol = ((a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]))
           + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])) / 6.0
    return area, vol


def mesh_components(verts, faces):
    """dict: comp int32 [F]; counts int64 [C, 5]; measures float64 [C, 8] (area and volume by math.fsum); abs_area, abs_volume
    [C] (the fsum of the terms' magnitudes: the scale of the summation bound); report [8]"""
    p = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = p.shape[0], f.shape[0]
    report = np.zeros(8, np.int64)
    report[0] = V | (F << 32)
    report[4] = V
    if F == 0:
        return dict(comp=np.zeros(0, np.int32), counts=np.zeros((0, 5), np.int64), measures=np.zeros((0, 8)), abs_area=np.zeros(0),
                    abs_volume=np.zeros(0), report=report)
    root = union_find(V, np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]]))
    froot = root[f[:, 0]]
    first = {}
    for i, r in enumerate(froot.tolist()):                  # the smallest face id of every root: the order of the components
        first.setdefault(r, i)
    roots = sorted(first, key=first.get)
    C = len(roots)
    vrank = np.full(V, -1, np.int64)
    used = np.zeros(V, bool)
    used[f.reshape(-1)] = True
    rank_of = np.full(V, -1, np.int64)
    rank_of[roots] = np.arange(C)
    vrank[used] = rank_of[root[used]]
    comp = rank_of[froot]
    counts = np.zeros((C, 5), np.int64)
    counts[:, 0] = [first[r] for r in roots]
    counts[:, 1] = np.bincount(comp, minlength=C)
    counts[:, 2] = np.bincount(vrank[used], minlength=C)
    # undirected pairs a != b, once per face that uses them
    e = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1)                         # [F, 3, 2]
    lo, hi = e.min(-1), e.max(-1)
    key = lo * (V + 1) + hi
    fid = np.repeat(np.arange(F)[:, None], 3, 1)
    ok = lo != hi
    per_face = np.unique(np.stack([fid[ok], key[ok]], 1), axis=0)                       # a face's repeated pair counts once
    ek, uses = np.unique(per_face[:, 1], return_counts=True)
    er = vrank[ek // (V + 1)]
    counts[:, 3] = np.bincount(er[uses == 1], minlength=C)
    counts[:, 4] = np.bincount(er[uses > 2], minlength=C)
    area, vol = face_terms(p, f)
    measures = np.zeros((C, 8))
    abs_area, abs_volume = np.zeros(C), np.zeros(C)
    order = np.argsort(comp, kind='stable')
    ends = np.cumsum(counts[:, 1])
    pd = p.astype(np.float64)
    for r in range(C):
        ids = order[ends[r] - counts[r, 1]:ends[r]]
        measures[r, 0] = math.fsum(area[ids].tolist())
        measures[r, 1] = math.fsum(vol[ids].tolist())
        abs_area[r] = measures[r, 0]
        abs_volume[r] = math.fsum(np.abs(vol[ids]).tolist())
    vorder = np.argsort(np.where(used, vrank, C), kind='stable')
    vends = np.cumsum(counts[:, 2])
    for r in range(C):
        q = pd[vorder[vends[r] - counts[r, 2]:vends[r]]]
        measures[r, 2:5] = q.min(0)
        measures[r, 5:8] = q.max(0)
    report[1] = C
    report[2] = counts[:, 1].max()
    report[3] = int(np.argmax(measures[:, 0]))              # the first of equal maxima
    report[4] = V - int(used.sum())
    return dict(comp=comp.astype(np.int32), counts=counts, measures=measures, abs_area=abs_area, abs_volume=abs_volume, report=report)


def stats(m):
    """the stats dict of points2surf_amd.components from the model's arrays"""
    c, q = m['counts'], m['measures']
    return dict(first_face=c[:, 0], faces=c[:, 1], vertices=c[:, 2], boundary_edges=c[:, 3], nonmanifold_edges=c[:, 4], area=q[:, 0],
                volume=q[:, 1], box_lo=q[:, 2:5], box_hi=q[:, 5:8], closed=(c[:, 3] == 0) & (c[:, 4] == 0))


def select(st, min_faces=0, min_area_share=0.0, max_components=0):
    """the rule of points2surf_amd.components.select, written as a loop"""
    area = [float(a) for a in st['area']]
    C = len(area)
    if C == 0:
        return np.zeros(0, bool)
    big = max(area)
    order = sorted(range(C), key=lambda c: (-area[c], int(st['first_face'][c])))
    keep = [int(st['faces'][c]) >= min_faces and area[c] >= np.float64(min_area_share) * np.float64(big) for c in range(C)]
    keep[order[0]] = True
    if max_components > 0:
        chosen = [c for c in order if keep[c]][:max_components]
        keep = [c in chosen for c in range(C)]
    return np.array(keep, bool)


def submesh(verts, faces, keep):
    """(verts, faces, face_src, vert_map) of the faces with keep != 0"""
    p = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    k = np.asarray(keep).reshape(-1) != 0
    used = np.zeros(p.shape[0], bool)
    used[f[k].reshape(-1)] = True
    vmap = np.where(used, np.cumsum(used) - 1, -1)
    return p[used], vmap[f[k]].astype(np.int32).reshape(-1, 3), np.flatnonzero(k).astype(np.int32), vmap.astype(np.int32)


# ---- clusters --------------------------------------------------------------------------------------------------------------

def linked_pairs(points, radius):
    """every pair i < j with (dx dx + dy dy) + dz dz <= radius * radius in float64, found over a grid of cells somewhat wider
    than the radius (neighbouring cells only)"""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    n = p.shape[0]
    if n < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    cell = np.floor((p - p.min(0)) / (float(radius) * 1.001)).astype(np.int64)
    dims = cell.max(0) + 3
    key = ((cell[:, 0] + 1) * dims[1] + (cell[:, 1] + 1)) * dims[2] + (cell[:, 2] + 1)
    order = np.argsort(key, kind='stable')
    skey = key[order]
    r2 = float(radius) * float(radius)
    out_a, out_b = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                want = key + (dx * dims[1] + dy) * dims[2] + dz
                s, e = np.searchsorted(skey, want, 'left'), np.searchsorted(skey, want, 'right')
                cnt = e - s
                i = np.repeat(np.arange(n), cnt)
                j = order[np.repeat(s, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
                m = i < j
                i, j = i[m], j[m]
                d = p[i] - p[j]
                near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2
                out_a.append(i[near])
                out_b.append(j[near])
    return np.concatenate(out_a), np.concatenate(out_b)


def clusters(points, radius, min_points):
    """dict: labels int32 [n] (the smallest point id of the cluster), ids int32 (the kept points, ascending), info int64 [4]"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    n = p.shape[0]
    info = np.zeros(4, np.int64)
    if n == 0:
        return dict(labels=np.zeros(0, np.int32), ids=np.zeros(0, np.int32), points=p, info=info)
    a, b = linked_pairs(p, radius)
    labels = union_find(n, a, b)
    size = np.bincount(labels, minlength=n)
    largest = int(size.max())
    least = min(int(min_points), largest)
    keep = size[labels] >= least
    roots = np.flatnonzero(size > 0)
    info[:] = [roots.size, largest, int(np.argmax(size)), int((size[roots] < least).sum())]
    ids = np.flatnonzero(keep).astype(np.int32)
    return dict(labels=labels.astype(np.int32), ids=ids, points=p[ids], info=info)


# ---- the cases of the tests ------------------------------------------------------------------------------------------------

def torus(nu, nv, R=0.35, r=0.14, centre=(0.0, 0.0, 0.0)):
    """a closed torus of nu x nv quads (2 nu nv faces), outward"""
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing='ij')
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return (p + np.asarray(centre, np.float64)).astype(np.float32), faces.astype(np.int32)


def join(meshes, seed=None):
    """the meshes under one index space; with a seed the face order and the vertex ids are seeded permutations"""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32).reshape(-1, 3))
        fs.append(np.asarray(f, np.int64).reshape(-1, 3) + base)
        base += vs[-1].shape[0]
    v, f = np.concatenate(vs), np.concatenate(fs)
    if seed is not None:
        rng = np.random.RandomState(seed)
        new_id = rng.permutation(v.shape[0])                # vertex i becomes new_id[i]
        v2 = np.empty_like(v)
        v2[new_id] = v
        v, f = v2, new_id[f][rng.permutation(f.shape[0])]
    return v, f.astype(np.int32)


def strip(n_faces, seed=3):
    """a triangle strip of n_faces faces whose face ids and vertex ids are a seeded permutation: deep parent chains"""
    k = np.arange(n_faces + 2)
    v = np.stack([k * 0.5, (k % 2) * 1.0, np.zeros(k.shape[0])], -1)
    f = np.stack([k[:-2], k[1:-1], k[2:]], -1)
    return join([(v, f)], seed=seed)


def separate_triangles(n):
    """n triangles that share nothing"""
    k = np.arange(n, dtype=np.float64)
    v = np.stack([np.stack([k, 0 * k, 0 * k], -1), np.stack([k + 0.5, 0 * k + 1, 0 * k], -1), np.stack([k, 0 * k, 0 * k + 1], -1)], 1)
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def tetra(scale=1.0, inward=False):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * scale
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)          # outward
    return v.astype(np.float32), f[:, ::-1].copy() if inward else f


def small_cases():
    """name -> (verts, faces): the hand-made meshes of the issue"""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    two = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], np.float32)
    fan = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, -1, 0]], np.float32)
    cases = {
        'empty': (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
        'vertices_only': (tri, np.zeros((0, 3), np.int32)),
        'one_face': (tri, np.array([[0, 1, 2]], np.int32)),
        'shared_vertex': (two, np.array([[0, 1, 2], [0, 3, 4]], np.int32)),
        'same_triangles_separate_indices': (np.concatenate([two, two[:1]]), np.array([[0, 1, 2], [5, 3, 4]], np.int32)),
        'unreferenced_at_both_ends': (np.concatenate([tri + 5, two, tri - 5]), np.array([[3, 4, 5], [3, 6, 7]], np.int32)),
        'repeated_index': (two, np.array([[1, 1, 2], [3, 4, 3], [0, 0, 0]], np.int32)),
        'quad': (quad, np.array([[0, 1, 2], [0, 2, 3]], np.int32)),
        'three_faces_on_one_edge': (fan, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32)),
        'tetra_with_cavity': join([tetra(1.0), tetra(0.25, inward=True)]),
        'strip2000': strip(2000),
    }
    for n in (63, 64, 65, 255, 256, 257):
        cases['strip%d' % n] = strip(n, seed=n)
        cases['separate%d' % n] = separate_triangles(n)
    return cases


def big_case(seed=11):
    """one closed component of 300,000 faces (a torus of 500 x 300 quads) with 40 closed blobs of 8 to 500 faces, the face
    order and the vertex ids permuted"""
    rng = np.random.RandomState(seed)
    meshes = [torus(500, 300)]
    shapes = [(2, 2), (10, 25)] + [(int(rng.randint(2, 16)), int(rng.randint(2, 17))) for _ in range(38)]
    for nu, nv in shapes:
        meshes.append(torus(nu, nv, R=0.01, r=0.004, centre=rng.uniform(-0.9, 0.9, 3)))
    return join(meshes, seed=seed)


def clump_cloud(seed=5):
    """a surface-like cloud of 20,000 points (a sphere of radius 0.5, spacing about 0.0125) plus three far clumps of 5, 50 and
    300 points; the radius 0.04 links the sphere and every clump, and nothing else"""
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(20000, 3))
    parts = [0.5 * d / np.linalg.norm(d, axis=1, keepdims=True)]
    for k, c in ((5, (1.5, 0, 0)), (50, (0, -1.5, 0.2)), (300, (-0.3, 0.4, 1.6))):
        parts.append(np.asarray(c) + rng.uniform(-0.02, 0.02, (k, 3)))
    p = np.concatenate(parts)
    return p[rng.permutation(p.shape[0])].astype(np.float32), 0.04


def cluster_cases():
    """name -> (points, radius)"""
    r = 5.0 / 8.0
    pair = np.array([[0, 0, 0], [3.0 / 8.0, 4.0 / 8.0, 0]], np.float32)
    far = pair.copy()
    far[1, 0] = np.nextafter(far[1, 0], np.float32(2))
    dirs = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float64)
    unit = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    rng = np.random.RandomState(9)
    chain = np.stack([np.arange(3000) * 0.999 * 0.01, np.zeros(3000), np.zeros(3000)], -1)[rng.permutation(3000)]
    g = np.arange(42)
    lattice = np.stack(np.meshgrid(g, g, g[:40], indexing='ij'), -1).reshape(-1, 3)[:70000] * 0.02
    cloud, cr = clump_cloud()
    cases = {
        'empty': (np.zeros((0, 3), np.float32), 1.0),
        'one': (np.ones((1, 3), np.float32), 1.0),
        'two_far': (np.array([[0, 0, 0], [3, 0, 0]], np.float32), 1.0),
        'exactly_radius': (pair, r),
        'one_ulp_further': (far, r),
        'star_inside': (np.concatenate([np.zeros((1, 3)), unit * 0.999]).astype(np.float32), 1.0),
        'star_outside': (np.concatenate([np.zeros((1, 3)), unit * 1.001]).astype(np.float32), 1.0),
        'coincident500': (np.full((500, 3), 0.25, np.float32), 0.1),
        'chain3000': (chain.astype(np.float32), 0.01),
        'lattice70000': (lattice.astype(np.float32), 0.01),
        'negative_coordinates': ((cloud[:4000] - 3.0).astype(np.float32), cr),
        'offset_1e4': ((chain[:500] * 100.0 + 1e4).astype(np.float32), 1.0),
        'clumps': (cloud, cr),
    }
    for n in (63, 64, 65, 257):
        cases['chain%d' % n] = (chain[:n].astype(np.float32), 0.05)
    return cases
