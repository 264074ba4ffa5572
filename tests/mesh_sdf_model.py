"""Float64 numpy model of the mesh-distance kernels (points2surf_amd/csrc/p2s_meshdist.hip, the handle's in
p2s_meshbuild.inl, the octree in p2s_mesh_octree.inl): the same operations in the
same association, so the device's squared distances are expected to agree to rounding of sqrt / division only.

* ``tri_closest``: closest point of a triangle by Ericson's regions (Real-Time Collision Detection 5.1.5) with the
  feature it lies on (0 face, 1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex a / b / c); a triangle whose |ab x ac|^2 is not
  above 2^-90 |ab|^2 |ac|^2 is measured as its three segments.
  The model restates the kernel's operations on purpose (that is what makes a 1e-13 comparison of d^2 meaningful), so it
  is NOT independent of the kernel for the region logic; the independent evidence is the reference's recorded distances
  (reproduced to 8e-6, the float32 rounding of its query points) and test_regions_agree_with_plane_projection.
* ``nearest``: exhaustive in effect, not in cost: every query against every triangle that can matter (triangles whose bounding sphere lies further than the
  nearest centroid plus a margin are skipped -- they can be neither the nearest nor a runner-up within the margin); ties go
  to the smallest face id.
* ``winding``: generalised winding number.
* ``MeshModel``: face normals, neighbours, angle-weighted vertex normals (2^-40 fixed point like the device), closedness,
  orientation, connected components; ``sign`` = pseudonormal sign with the device's "too small to trust" bound; ``signed_distance`` = the whole
  entry point (positive inside, d <= 1e-8 unsigned, flagged queries decided by the winding number;
  a mesh of 2..16 components, which may overlap, sums the components' pseudonormal signs into its winding number).
"""
import numpy as np

FIX = 2.0 ** 40
DEGENERATE_REL = 2.0 ** -90
SLIVER_REL = 2.0 ** -40         # on sin^2 of the smallest corner: the normal of such a face is not trusted
MERGE_TOL = 1e-8


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _seg_closest(P, A, B):
    ab, ap = B - A, P - A
    t, l = dot3(ab, ap), dot3(ab, ab)
    with np.errstate(all='ignore'):
        v = t / l
    c = A + v[:, None] * ab
    end = np.zeros(len(P), np.int64)
    lo, hi = t <= 0.0, (t >= l) & ~(t <= 0.0)
    c[lo], end[lo] = A[lo], 1
    c[hi], end[hi] = B[hi], 2
    r = P - c
    return dot3(r, r), c, end


def tri_closest(P, T):
    """P [K, 3], T [K, 9] float64 -> (d2 [K], closest [K, 3], feature [K])"""
    P = np.asarray(P, np.float64)
    T = np.asarray(T, np.float64)
    A, B, C = T[:, 0:3], T[:, 3:6], T[:, 6:9]
    ab, ac, ap = B - A, C - A, P - A
    n = cross3(ab, ac)
    deg = ~(dot3(n, n) > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)))
    d1, d2 = dot3(ab, ap), dot3(ac, ap)
    bp, cp = P - B, P - C
    d3, d4, d5, d6 = dot3(ab, bp), dot3(ac, bp), dot3(ab, cp), dot3(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    K = len(P)
    c = np.empty((K, 3))
    feat = np.full(K, -1, np.int64)

    def put(mask, val, code):
        mk = mask & (feat < 0)
        c[mk] = val[mk]
        feat[mk] = code

    with np.errstate(all='ignore'):
        put((d1 <= 0) & (d2 <= 0), A, 4)
        put((d3 >= 0) & (d4 <= d3), B, 5)
        v = d1 / (d1 - d3)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), A + v[:, None] * ab, 1)
        put((d6 >= 0) & (d5 <= d6), C, 6)
        w = d2 / (d2 - d6)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), A + w[:, None] * ac, 3)
        w2 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), B + w2[:, None] * (C - B), 2)
        den = 1.0 / ((va + vb) + vc)
        put(np.ones(K, bool), (A + ab * (vb * den)[:, None]) + ac * (vc * den)[:, None], 0)
    r = P - c
    dd = dot3(r, r)
    if deg.any():
        i = np.nonzero(deg)[0]
        best, cb, e = _seg_closest(P[i], A[i], B[i])
        fb = np.where(e == 0, 1, 3 + e)
        d, c2, e2 = _seg_closest(P[i], B[i], C[i])
        m = d < best
        best, cb, fb = np.where(m, d, best), np.where(m[:, None], c2, cb), np.where(m, np.where(e2 == 0, 2, 4 + e2), fb)
        d, c2, e2 = _seg_closest(P[i], C[i], A[i])
        m = d < best
        best, cb = np.where(m, d, best), np.where(m[:, None], c2, cb)
        fb = np.where(m, np.where(e2 == 0, 3, np.where(e2 == 1, 6, 4)), fb)
        dd[i], c[i], feat[i] = best, cb, fb
    return dd, c, feat


def nearest(verts, faces, queries, chunk=128, margin=1e-3):
    """-> d2 [n], face [n] (smallest id among ties), closest [n, 3], feature [n], runner-up d2 [n] (inf if none within
    the margin)"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    q = np.asarray(queries, np.float64)
    tri = v[f].reshape(len(f), 9)
    cen = v[f].mean(1)
    rad = np.sqrt(((v[f] - cen[:, None, :]) ** 2).sum(-1)).max(1)
    n = len(q)
    out_d2, out_f, out_c = np.full(n, np.inf), np.full(n, -1, np.int64), np.full((n, 3), np.nan)
    out_feat, out_second = np.full(n, -1, np.int64), np.full(n, np.inf)
    for s in range(0, n, chunk):
        qq = q[s:s + chunk]
        D = np.sqrt(((qq[:, None, :] - cen[None, :, :]) ** 2).sum(-1))
        ub = D.min(1)                                    # the nearest centroid is a point of the mesh
        qi, fi = np.nonzero(D - rad[None, :] <= (ub * (1 + 1e-9) + margin)[:, None])
        d2, c, feat = tri_closest(qq[qi], tri[fi])
        order = np.lexsort((fi, d2, qi))
        qi_o = qi[order]
        first = np.nonzero(np.r_[True, qi_o[1:] != qi_o[:-1]])[0]
        rows = qi_o[first] + s
        out_d2[rows], out_f[rows], out_c[rows], out_feat[rows] = d2[order][first], fi[order][first], c[order][first], feat[order][first]
        nxt = first + 1
        has = (nxt < len(qi_o)) & (qi_o[np.minimum(nxt, len(qi_o) - 1)] == qi_o[first])
        out_second[rows[has]] = d2[order][nxt[has]]
    return out_d2, out_f, out_c, out_feat, out_second


def winding(queries, tri, chunk=64):
    """generalised winding number of every query: sum of 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 4 pi"""
    q = np.asarray(queries, np.float64)
    T = np.asarray(tri, np.float64).reshape(-1, 9)
    out = np.empty(len(q))
    for s in range(0, len(q), chunk):
        P = q[s:s + chunk, None, :]
        a, b, c = T[None, :, 0:3] - P, T[None, :, 3:6] - P, T[None, :, 6:9] - P
        la, lb, lc = np.sqrt(dot3(a, a)), np.sqrt(dot3(b, b)), np.sqrt(dot3(c, c))
        num = dot3(a, cross3(b, c))
        den = ((la * lb * lc + dot3(a, b) * lc) + dot3(b, c) * la) + dot3(c, a) * lb
        out[s:s + chunk] = np.arctan2(num, den).sum(-1) / (2 * np.pi)
    return out


def edge_census(faces, n_verts):
    """(undirected edge keys, traversals low -> high, traversals high -> low)"""
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    key = np.minimum(a, b) * n_verts + np.maximum(a, b)
    uk, inv = np.unique(key, return_inverse=True)
    fwd = np.bincount(inv[a < b], minlength=len(uk))
    bwd = np.bincount(inv[~(a < b)], minlength=len(uk))
    return uk, fwd, bwd


class MeshModel:
    def __init__(self, verts, faces):
        v = np.asarray(verts, np.float32).astype(np.float64)
        f = np.asarray(faces, np.int64)
        self.n_verts = len(v)
        _, fwd, bwd = edge_census(f, len(v))
        self.bad_edges = int((~((fwd == 1) & (bwd == 1))).sum())
        self.closed = self.bad_edges == 0
        vol6 = dot3(v[f[:, 0]], cross3(v[f[:, 1]], v[f[:, 2]])).sum()
        self.inverted = bool(self.closed and vol6 < 0)
        if self.inverted:
            f = f[:, [0, 2, 1]]
        self.verts, self.faces = v, f
        self.tri = v[f].reshape(len(f), 9)
        A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        ab, ac = B - A, C - A
        n = cross3(ab, ac)
        nn = dot3(n, n)
        deg = ~(nn > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)))
        with np.errstate(all='ignore'):
            inv = np.where(deg, 0.0, 1.0 / np.sqrt(nn))
        self.fn = np.where(deg[:, None], 0.0, n * inv[:, None])
        bc = C - B
        l0, l1, l2 = dot3(ab, ab), dot3(ac, ac), dot3(bc, bc)
        with np.errstate(all='ignore'):
            self.fbad = deg | ~(nn > SLIVER_REL * ((l0 * l1 * l2) / np.minimum(l0, np.minimum(l1, l2))))
        self.vbad = np.zeros(len(v), bool)
        self.vbad[f[self.fbad].reshape(-1)] = True
        # neighbours across ab, bc, ca
        self.adj = np.full((len(f), 3), -1, np.int64)
        if self.closed:
            a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
            b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
            face = np.tile(np.arange(len(f)), 3)
            slot = np.repeat(np.arange(3), len(f))
            key = np.minimum(a, b) * len(v) + np.maximum(a, b)
            order = np.argsort(key, kind='stable')
            p0, p1 = order[0::2], order[1::2]
            self.adj[face[p0], slot[p0]] = face[p1]
            self.adj[face[p1], slot[p1]] = face[p0]
        # connected components over the neighbours (closed meshes): min-label propagation
        self.components = 0
        if self.closed:
            lab = np.arange(len(f))
            while True:
                new = np.minimum(lab, lab[self.adj].min(1))
                new = new[new]
                if np.array_equal(new, lab):
                    break
                lab = new
            self.components = len(np.unique(lab))
            self.comp = lab                      # label of a component = its smallest face id
        # angle-weighted vertex normals, 2^-40 fixed point
        vn = np.zeros((len(v), 4), np.int64)
        P = [A, B, C]
        for j in range(3):
            u, w = P[(j + 1) % 3] - P[j], P[(j + 2) % 3] - P[j]
            x = cross3(u, w)
            ang = np.arctan2(np.sqrt(dot3(x, x)), dot3(u, w))
            ok = ~deg
            for k in range(3):
                np.add.at(vn[:, k], f[ok, j], np.rint(ang[ok] * self.fn[ok, k] * FIX).astype(np.int64))
            np.add.at(vn[:, 3], f[ok, j], np.rint(ang[ok] * FIX).astype(np.int64))
        self.vn = vn
        self.scale = float(np.abs(v).max())

    def nearest(self, queries):
        return nearest(self.verts, self.faces, queries)

    def sign(self, queries, face, closest, feat, d):
        """-> (outside [n] bool, flagged [n] bool): pseudonormal sign and the "too small to trust" flag"""
        q = np.asarray(queries, np.float64)
        n = np.empty((len(q), 3))
        W = np.empty(len(q))
        isf, ise, isv = feat == 0, (feat >= 1) & (feat <= 3), feat >= 4
        untrusted = self.fbad[face].copy()
        n[isf], W[isf] = self.fn[face[isf]], 1.0
        g = self.adj[face[ise], feat[ise] - 1]
        untrusted[ise] |= (g < 0) | self.fbad[np.maximum(g, 0)]
        n[ise] = self.fn[face[ise]] + np.where((g >= 0)[:, None], self.fn[np.maximum(g, 0)], 0.0)
        W[ise] = 2.0
        vid = self.faces[face[isv], feat[isv] - 4]
        n[isv], W[isv] = self.vn[vid, :3].astype(np.float64) / FIX, self.vn[vid, 3].astype(np.float64) / FIX
        untrusted[isv] |= self.vbad[vid]
        r = q - closest
        dt = dot3(n, r)
        s = np.maximum(self.scale, np.abs(q).max(1))
        bound = 2.0 ** -30 * (W * d) + 2.0 ** -45 * (np.sqrt(dot3(n, n)) * s)
        return dt > 0.0, untrusted | ~(np.abs(dt) > bound)

    def pseudonormal_sign(self, queries, nearest_all=None):
        """-> (inside [n], untrusted [n]).  One component: the pseudonormal of the nearest feature.  2..16 components (they
        may overlap): the winding number is the sum over the components, w = sum_k o_k [inside component k], o_k the sign
        of the component's own volume, the bracket from the pseudonormal of the nearest feature of THAT component;
        inside iff w != 0.  untrusted: a dot product within the bound, or the query on a component (d_k <= 1e-8)."""
        q = np.asarray(queries, np.float64)
        if self.components <= 1:
            d2, face, c, feat, _ = nearest_all if nearest_all is not None else self.nearest(q)
            outside, flagged = self.sign(q, face, c, feat, np.sqrt(d2))
            return ~outside, flagged
        wsum, bad = np.zeros(len(q), np.int64), np.zeros(len(q), bool)
        for root in np.unique(self.comp):
            idx = np.nonzero(self.comp == root)[0]
            t = self.tri[idx]
            o = -1 if dot3(t[:, 0:3], cross3(t[:, 3:6], t[:, 6:9])).sum() < 0 else 1
            d2, local, c, feat, _ = nearest(self.verts, self.faces[idx], q)
            outside, flagged = self.sign(q, idx[local], c, feat, np.sqrt(d2))
            bad |= flagged | (np.sqrt(d2) <= MERGE_TOL)
            wsum += np.where(outside if o < 0 else ~outside, o, 0)
        return wsum != 0, bad

    def signed_distance(self, queries, with_details=False):
        q = np.asarray(queries, np.float64)
        d2, face, c, feat, second = self.nearest(q)
        d = np.sqrt(d2)
        if self.components > 16:         # every sign from the winding number
            outside, flagged = np.zeros(len(q), bool), np.ones(len(q), bool)
        else:
            inside, flagged = self.pseudonormal_sign(q, (d2, face, c, feat, second))
            outside = ~inside
        flagged = flagged & (d > MERGE_TOL)
        if flagged.any():
            outside[flagged] = ~(np.abs(winding(q[flagged], self.tri)) > 0.5)
        out = np.where(outside & (d > MERGE_TOL), -d, d)
        if with_details:
            return out, dict(d2=d2, face=face, closest=c, feat=feat, second=second, flagged=flagged)
        return out


def query_dist_post(d):
    """make_dataset.py:467-474: NaN -> 0, inf -> 1, clamp to [-1, 1], float32"""
    d = np.array(d, np.float64)
    nan, inf = np.isnan(d), np.isinf(d)
    d[nan] = 0.0
    d[inf] = 1.0
    d[d < -1.0] = -1.0
    d[d > 1.0] = 1.0
    return d.astype(np.float32)


def l_prism():
    """closed, outward-oriented L-shaped prism: convex edges, one reflex edge (x = y = 1), convex vertices"""
    poly = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], np.float32)
    v = np.concatenate([np.c_[poly, np.zeros(6)], np.c_[poly, np.ones(6)]]).astype(np.float32)
    cap = [(0, 1, 2), (0, 2, 3), (0, 3, 5), (3, 4, 5)]
    f = [(a + 6, b + 6, c + 6) for a, b, c in cap] + [(a, c, b) for a, b, c in cap]
    for i in range(6):
        j = (i + 1) % 6
        f += [(i, j, j + 6), (i, j + 6, i + 6)]
    return v, np.array(f, np.int32)
