"""Float64 numpy model of p2s_mesh_render (points2surf_amd/csrc/p2s_meshrender.inl; the definition: include/p2s_hip.h): the
same operations in the same association, contraction off, so the device's bytes, depth bits, face ids and counters are
expected to EQUAL the model's.

* ``sample_rays``: the rays of the (W ss) x (H ss) sample image, entry Y (W ss) + X.
* first hit: every ray against every triangle (``scan_model.hit_table``), the smallest t, ties to the smallest face id.
* occlusion: every occlusion ray against every triangle with t_max = ao_radius; occluded iff any pair hits.
* shading, resolve and encoding as the header states them.
* ``Octree``: the handle's index (the choice of G, the cell of every centroid in float32, ascending face ids per cell, the
  float32 boxes) and both walks of it on the host, one ray at a time, with the acceptance taken from the exhaustive table.
  It gives the ray-triangle tests that the device counts (stats[4]) and checks the skip argument on the way: a walk whose
  answer differed from the exhaustive one would fail the model's own assertion.
The handle's arrays (stored corner order of an inward-oriented closed mesh, unit face normals, fixed-point vertex normals, the
sliver flags) are ``mesh_sdf_model.MeshModel``'s."""
import math
import struct
import zlib

import numpy as np

import scan_model as SM
from mesh_sdf_model import FIX, MeshModel, cross3, dot3

INF = float('inf')
DEFAULTS = dict(width=8, height=8, samples=1, projection=0, shading=0, ao_rays=0, eye=(0.0, 0.0, 3.0), right=(1.0, 0.0, 0.0),
                up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, -1.0), tan_half_w=0.5, tan_half_h=0.5, half_w=1.0, half_h=1.0, ao_radius=0.5,
                ao_bias=1.0 / 1024.0, ambient=0.6, diffuse=0.4, base_rgb=(0.8, 0.8, 0.8), background_rgb=(1.0, 1.0, 1.0))


def params(**kw):
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """dict(eye, right, up, forward): an orthonormal frame looking from ``eye`` at ``target``"""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    f = target - eye
    f = f / math.sqrt(float(f @ f))
    r = np.cross(f, up)
    r = r / math.sqrt(float(r @ r))
    u = np.cross(r, f)
    u = u / math.sqrt(float(u @ u))
    return dict(eye=tuple(eye), right=tuple(r), up=tuple(u), forward=tuple(f))


def sample_rays(p):
    """[H ss * W ss, 6] float64"""
    W, H, ss = p['width'], p['height'], p['samples']
    X, Y = np.arange(W * ss), np.arange(H * ss)
    i, a, j, b = X // ss, X % ss, Y // ss, Y % ss
    sx = (2.0 * (i.astype(np.float64) + (a.astype(np.float64) + 0.5) / float(ss))) / float(W) - 1.0
    sy = 1.0 - (2.0 * (j.astype(np.float64) + (b.astype(np.float64) + 0.5) / float(ss))) / float(H)
    pin = p['projection'] == 0
    kx = np.broadcast_to((sx * (p['tan_half_w'] if pin else p['half_w']))[None, :, None], (H * ss, W * ss, 1))
    ky = np.broadcast_to((sy * (p['tan_half_h'] if pin else p['half_h']))[:, None, None], (H * ss, W * ss, 1))
    eye, right, up, fwd = (np.asarray(p[k], np.float64).reshape(1, 1, 3) for k in ('eye', 'right', 'up', 'forward'))
    moved = lambda base: (base + kx * right) + ky * up
    o = np.broadcast_to(eye, (H * ss, W * ss, 3)) if pin else moved(eye)
    d = moved(fwd) if pin else np.broadcast_to(fwd, (H * ss, W * ss, 3))
    return np.concatenate([o, d], -1).reshape(-1, 6)


class Octree:
    """the index of p2s_trimesh_create over a MeshModel, and the two walks of it"""

    def __init__(self, mm):
        F = len(mm.faces)
        L = 1
        while L < 7 and float(1 << L) * float(1 << L) * 8.0 < float(F):
            L += 1
        G = 1 << L
        v32 = mm.verts.astype(np.float32)
        lo, hi = v32.min(0), v32.max(0)
        ext = np.float32(max(hi - lo))
        if not ext > 0:
            ext = np.float32(1.0)
        inv_cell = np.float32(G) / ext
        T = mm.tri
        c = (((T[:, 0:3] + T[:, 3:6]) + T[:, 6:9]) / 3.0).astype(np.float32)
        ci = np.clip(((c - lo) * inv_cell).astype(np.int32), 0, G - 1).astype(np.int64)
        cell = (ci[:, 0] * G + ci[:, 1]) * G + ci[:, 2]
        self.L, self.G, self.scale = L, G, mm.scale
        self.leaf = [[] for _ in range(G ** 3)]
        for f in range(F):                                   # ascending face ids per cell
            self.leaf[int(cell[f])].append(f)
        P = T.reshape(F, 3, 3)
        blo = np.full((G ** 3, 3), np.inf)
        bhi = np.full((G ** 3, 3), -np.inf)
        np.minimum.at(blo, cell, P.min(1))
        np.maximum.at(bhi, cell, P.max(1))
        self.lo, self.hi = [None] * (L + 1), [None] * (L + 1)
        self.lo[L], self.hi[L] = blo, bhi
        for l in range(L - 1, -1, -1):                       # lin = (x n + y) n + z
            n = 1 << l
            shape = (n, 2, n, 2, n, 2, 3)
            self.lo[l] = self.lo[l + 1].reshape(shape).min((1, 3, 5)).reshape(-1, 3)
            self.hi[l] = self.hi[l + 1].reshape(shape).max((1, 3, 5)).reshape(-1, 3)
        self.lo = [x.tolist() for x in self.lo]
        self.hi = [x.tolist() for x in self.hi]

    def _reaches(self, l, lin, o, d, inv, g, limit):
        lo, hi = self.lo[l][lin], self.hi[l][lin]
        if lo[0] > hi[0]:
            return False
        entry, exit_ = 0.0, INF
        for k in range(3):
            a, b = lo[k] - g, hi[k] + g
            if d[k] == 0.0:
                if not (o[k] >= a and o[k] <= b):
                    return False
            else:
                t1, t2 = (a - o[k]) * inv[k], (b - o[k]) * inv[k]
                entry = max(entry, min(t1, t2))
                exit_ = min(exit_, max(t1, t2))
        return entry <= exit_ and entry < INF and entry <= limit

    def walk(self, ray, limit, row, first_hit):
        """``first_hit``: ``row`` [F] = t of the ray on every face (inf: no hit) -> (t, face, tests) of p2s_mr_index_kernel.
        Else ``row`` [F] bool = the face is hit within (0, limit] -> (occluded, tests) of the any-hit walk."""
        o = [float(x) for x in ray[0:3]]
        d = [0.0 if abs(float(x)) < SM.TINY else float(x) for x in ray[3:6]]
        fin = all(abs(x) <= SM.BIG for x in o + d)           # false for NaN
        if not (fin and any(x != 0.0 for x in d) and limit > 0.0):
            return (INF, -1, 0) if first_hit else (False, 0)
        g = 2.0 * (max(self.scale, max(abs(x) for x in o)) * SM.RAY_BOX_REL)
        inv = [1.0 / x if x != 0.0 else INF for x in d]
        m = 0
        for k in range(3):
            m = (m << 1) | (1 if d[k] < 0.0 else 0)
        best, bestf, tests = INF, -1, 0
        stack = [(0, 0)]
        while stack:
            l, lin = stack.pop()
            if first_hit and not self._reaches(l, lin, o, d, inv, g, min(best, limit)):
                continue
            if l == self.L:
                for f in self.leaf[lin]:
                    tests += 1
                    if not first_hit:
                        if row[f]:
                            return True, tests
                    else:
                        th = row[f]
                        if th < best or (th == best and th < INF and f < bestf):
                            best, bestf = th, f
            else:
                n = 1 << l
                x, y, z = lin >> (2 * l), (lin >> l) & (n - 1), lin & (n - 1)
                for j in range(7, -1, -1):
                    c = j ^ m
                    clin = ((2 * x + (c >> 2)) * (2 * n) + (2 * y + ((c >> 1) & 1))) * (2 * n) + (2 * z + (c & 1))
                    if self._reaches(l + 1, clin, o, d, inv, g, min(best, limit) if first_hit else limit):
                        stack.append((l + 1, clin))
        return (best, bestf, tests) if first_hit else (False, tests)


def _chunks(n, F):
    step = max(1, int(1.5e6 // max(F, 1)))
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def first_hits(mm, tree, rays):
    """(t [n], face [n], tests): exhaustive first hit; the index walk must give the same"""
    n = len(rays)
    t_out, f_out, tests = np.full(n, np.inf), np.full(n, -1, np.int64), 0
    for a, b in _chunks(n, len(mm.tri)):
        tab = SM.hit_table(mm.tri, rays[a:b], np.inf, mm.scale)
        f = tab.argmin(1)
        t = tab[np.arange(b - a), f]
        t_out[a:b], f_out[a:b] = t, np.where(t < np.inf, f, -1)
        if tree is not None:
            for r in range(a, b):
                wt, wf, k = tree.walk(rays[r], INF, tab[r - a], True)
                assert wt == t_out[r] and wf == f_out[r], (r, wt, wf, t_out[r], f_out[r])
                tests += k
    return t_out, f_out, tests


def any_hits(mm, tree, rays, limit):
    """(occluded [n] bool, tests)"""
    n = len(rays)
    occ, tests = np.zeros(n, bool), 0
    for a, b in _chunks(n, len(mm.tri)):
        tab = SM.hit_table(mm.tri, rays[a:b], limit, mm.scale) < np.inf
        occ[a:b] = tab.any(1)
        if tree is not None:
            for r in range(a, b):
                got, k = tree.walk(rays[r], limit, tab[r - a], False)
                assert got == occ[r], (r, got, occ[r])
                tests += k
    return occ, tests


def encode(x):
    """byte = floor(255 sqrt(x) + 1/2)"""
    return np.floor(255.0 * np.sqrt(x) + 0.5).astype(np.uint8)


def render(verts, faces, p, vertex_rgb=None, ao_dirs=None, count_tests=True):
    """dict: rgb uint8 [H, W, 3], depth float64 and face int32 [H ss, W ss], stats int64 [8], and the per-sample parts
    (colour [H ss, W ss, 3], ao [n] with 1 on a miss, normal [n, 3], lambert [n]) for the closed-form tests"""
    mm = MeshModel(verts, faces)
    tree = Octree(mm) if count_tests else None
    W, H, ss, K = p['width'], p['height'], p['samples'], p['ao_rays']
    rays = sample_rays(p)
    n = len(rays)
    t, face, tests = first_hits(mm, tree, rays)
    hit = face >= 0
    col = np.empty((n, 3))
    col[:] = np.fmin(np.fmax(np.asarray(p['background_rgb'], np.float64), 0.0), 1.0)
    ao_all, nrm_all, lam_all = np.ones(n), np.zeros((n, 3)), np.zeros(n)
    occluded = 0
    if hit.any():
        f = face[hit]
        o, d, th = rays[hit, 0:3], rays[hit, 3:6].copy(), t[hit]
        d[np.abs(d) < SM.TINY] = 0.0
        P = mm.tri[f]
        A, e1, e2 = P[:, 0:3], P[:, 3:6] - P[:, 0:3], P[:, 6:9] - P[:, 0:3]
        nf = cross3(e1, e2)
        s = o - A
        q = cross3(s, d)
        dn = dot3(d, nf)
        u, v = -dot3(e2, q) / dn, dot3(e1, q) / dn
        w0 = (1.0 - u) - v
        vi = mm.faces[f]
        nrm = mm.fn[f].copy()
        if p['shading'] == 1:
            N = mm.vn[:, 0:3].astype(np.float64) / FIX
            m = (w0[:, None] * N[vi[:, 0]] + u[:, None] * N[vi[:, 1]]) + v[:, None] * N[vi[:, 2]]
            mq = dot3(m, m)
            ok = ~mm.vbad[vi].any(1) & (mq > 0.0) & (mq <= 1.0e300)
            with np.errstate(all='ignore'):
                nrm = np.where(ok[:, None], m / np.sqrt(mq)[:, None], nrm)
        dl = d / np.sqrt(dot3(d, d))[:, None]
        c = dot3(nrm, dl)
        flip = c > 0.0
        nrm = np.where(flip[:, None], -nrm, nrm)
        lambert = -np.where(flip, -c, c)
        if vertex_rgb is not None:
            C = np.asarray(vertex_rgb, np.float32).astype(np.float64)
            with np.errstate(all='ignore'):
                alb = (w0[:, None] * C[vi[:, 0]] + u[:, None] * C[vi[:, 1]]) + v[:, None] * C[vi[:, 2]]
        else:
            alb = np.broadcast_to(np.asarray(p['base_rgb'], np.float64), (len(f), 3))
        ao = np.ones(len(f))
        if K > 0:
            h = np.asarray(ao_dirs, np.float64).reshape(K, 3)
            nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
            sg = np.copysign(1.0, nz)
            ia = -1.0 / (sg + nz)
            ib = (nx * ny) * ia
            t1 = np.stack([1.0 + ((sg * nx) * nx) * ia, sg * ib, -(sg * nx)], 1)
            t2 = np.stack([ib, sg + (ny * ny) * ia, -ny], 1)
            po = (o + th[:, None] * d) + p['ao_bias'] * nrm
            dirs = (h[None, :, 0:1] * t1[:, None, :] + h[None, :, 1:2] * t2[:, None, :]) + h[None, :, 2:3] * nrm[:, None, :]
            ao_rays = np.concatenate([np.broadcast_to(po[:, None, :], dirs.shape), dirs], -1).reshape(-1, 6)
            occ, k = any_hits(mm, tree, ao_rays, p['ao_radius'])
            tests += k
            occ = occ.reshape(len(f), K).sum(1)
            occluded = int(occ.sum())
            ao = (K - occ).astype(np.float64) / float(K)
        shade = p['ambient'] * ao + p['diffuse'] * lambert
        with np.errstate(all='ignore'):
            col[hit] = np.fmin(np.fmax(alb * shade[:, None], 0.0), 1.0)
        ao_all[hit], nrm_all[hit], lam_all[hit] = ao, nrm, lambert
    img = col.reshape(H * ss, W * ss, 3)
    acc = np.zeros((H, W, 3))
    for b in range(ss):
        for a in range(ss):
            acc = acc + img[b::ss, a::ss]
    rgb = encode(acc / float(ss * ss))
    n_hit = int(hit.sum())
    stats = np.array([n, n_hit, n_hit * K, occluded, tests, 0, 0, 0], np.int64)
    return dict(rgb=rgb, depth=t.reshape(H * ss, W * ss), face=face.astype(np.int32).reshape(H * ss, W * ss), stats=stats, rays=rays,
                colour=img, ao=ao_all, normal=nrm_all, lambert=lam_all, inverted=mm.inverted)


def decode_png(data):
    """8-bit RGB, filter 0 on every row: uint8 [H, W, 3]"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(data):
        n, = struct.unpack('>I', data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b''.join(b for k, b in chunks if k == b'IDAT'))
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3)


# ---- meshes of the tests
def icosphere(subdivisions, radius=1.0):
    """(verts float32 [V, 3], faces int32 [20 * 4^s, 3]), outward"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / math.sqrt(1.0 + g * g) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / math.sqrt(float(p @ p)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def cube(h=1.0):
    """the axis-aligned cube [-h, h]^3, outward, 12 faces"""
    v = np.array([(x, y, z) for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)
    f = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                  (1, 5, 7), (1, 7, 3)], np.int32)
    return v, f


def sheet(n=4, h=1.0, z=0.0):
    """an open sheet of n x n quads in the plane ``z``, normal +z"""
    g = np.linspace(-h, h, n + 1)
    v = np.array([(x, y, z) for y in g for x in g], np.float32)
    f = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            f += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return v, np.array(f, np.int32)


def floor_and_plate(gap=0.25, plate=0.5):
    """a floor [-2, 2]^2 at z = 0 and a plate [-plate, plate]^2 at z = gap above its middle, both facing +z"""
    v0, f0 = sheet(4, 2.0, 0.0)
    v1, f1 = sheet(1, plate, gap)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)]).astype(np.int32)


def merged(*meshes):
    vs, fs, at = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int32) + at)
        at += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)
