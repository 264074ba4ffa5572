"""float64 restatement of the Screened Poisson baseline (include/p2s_hip.h) with scipy.sparse: the box,
the levels, W, the 1-D matrices, A and b as Kronecker products, the cascade solved to 1e-12, iso, the volume with its
border rule.  The yardstick of points2surf_amd/csrc/p2s_poisson.hip; also the sums over absolute values that bound the
rounding of the device's float32 pieces.  Level (sparse, Kronecker products) is the definition; FreeLevel applies the same
operators separably, for the depths at which the products are out of reach; one_step_cascade is the cascade cut after one CG
step per level, in float64 and with the device's float32 stores."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

MIN_DEPTH = 3


def box(points, scale):
    """(lo [3], side): centre = midpoint of the bounding box, side = scale * largest extent, float64"""
    p = np.asarray(points, np.float32).astype(np.float64)
    mn, mx = p.min(axis=0), p.max(axis=0)
    centre = (mn + mx) / 2.0
    side = scale * (mx - mn).max()
    return centre - side / 2.0, side


def cells(points, lo, h, R):
    """(cell [n, 3] int, t [n, 3]) with cell = clamp(floor((p - lo) / h), 0, R - 2)"""
    g = (np.asarray(points, np.float32).astype(np.float64) - lo) / h
    c = np.clip(np.floor(g), 0, R - 2).astype(np.int64)
    return c, g - c


def weights(points, lo, h, R):
    """W [n, R^3] csr, trilinear; the flat cell ids"""
    c, t = cells(points, lo, h, R)
    n = c.shape[0]
    rows, cols, vals = [], [], []
    for k in range(8):
        kx, ky, kz = k >> 2, (k >> 1) & 1, k & 1
        w = (t[:, 0] if kx else 1.0 - t[:, 0]) * (t[:, 1] if ky else 1.0 - t[:, 1]) * (t[:, 2] if kz else 1.0 - t[:, 2])
        rows.append(np.arange(n))
        cols.append(((c[:, 0] + kx) * R + c[:, 1] + ky) * R + c[:, 2] + kz)
        vals.append(w)
    W = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, R ** 3))
    return W, (c[:, 0] * (R - 1) + c[:, 1]) * (R - 1) + c[:, 2]


def m1(i, j, R, h):
    """1-D mass matrix, natural ends"""
    if i == j:
        return h / 3.0 if i in (0, R - 1) else 2.0 * h / 3.0
    return h / 6.0 if abs(i - j) == 1 else 0.0


def s1(i, j, R, h):
    """1-D stiffness matrix, natural ends"""
    if i == j:
        return 1.0 / h if i in (0, R - 1) else 2.0 / h
    return -1.0 / h if abs(i - j) == 1 else 0.0


def g1(i, j, R, h):
    """g[i][j] = integral of B_i' B_j"""
    if j == i + 1:
        return -0.5
    if j == i - 1:
        return 0.5
    if i == j:
        return -0.5 if i == 0 else (0.5 if i == R - 1 else 0.0)
    return 0.0


def mats_1d(R, h):
    def build(fn):
        i = np.arange(R)
        rows = np.concatenate([i, i[:-1], i[1:]])
        cols = np.concatenate([i, i[1:], i[:-1]])
        vals = [fn(int(a), int(b), R, h) for a, b in zip(rows, cols)]
        return sp.csr_matrix((vals, (rows, cols)), shape=(R, R))
    return build(m1), build(s1), build(g1)


def kron3(a, b, c):
    return sp.kron(a, sp.kron(b, c, format='csr'), format='csr')


class Level:
    """one level's system: R, h, lo, W, n_occ, a, lam, A, b, diag and the |.| companions"""

    def __init__(self, points, normals, depth, point_weight=4.0, scale=1.1):
        lo, side = box(points, scale)
        self.lo, self.R, self.h = lo, 2 ** depth + 1, side / 2 ** depth
        R, h = self.R, self.h
        nrm = np.asarray(normals, np.float32).astype(np.float64)
        n = nrm.shape[0]
        self.W, cell = weights(points, lo, h, R)
        self.n_occ = int(np.unique(cell).size)
        self.a = self.n_occ * h * h / n
        self.lam = point_weight * self.a / h
        m, s, g = mats_1d(R, h)
        self.v = (self.a / h ** 3) * (self.W.T @ (-nrm))
        self.v_abs = (self.a / h ** 3) * (self.W.T @ np.abs(nrm))
        G = (kron3(g, m, m), kron3(m, g, m), kron3(m, m, g))
        self.b = sum(G[a] @ self.v[:, a] for a in range(3))
        self.b_abs = sum(abs(G[a]) @ self.v_abs[:, a] for a in range(3))
        self.A0 = kron3(s, m, m) + kron3(m, s, m) + kron3(m, m, s)
        self.A0_abs = kron3(abs(s), m, m) + kron3(m, abs(s), m) + kron3(m, m, abs(s))
        self.WtW = (self.W.T @ self.W).tocsr()
        self.A = (self.A0 + self.lam * self.WtW).tocsr()
        self.diag = self.A.diagonal()

    def apply(self, x):
        return self.A @ np.asarray(x, np.float64).reshape(-1)

    def apply_abs(self, x):
        """the sum over the absolute values of the terms of A x"""
        ax = np.abs(np.asarray(x, np.float64).reshape(-1))
        return self.A0_abs @ ax + self.lam * (self.WtW @ ax)


def _f32(x):
    """rounded to float32, held as float64"""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _same(x):
    return x


def tri_1d(R, h, rnd=_same):
    """the 1-D matrices as (diagonal [R], the coefficient of x[i - 1], the coefficient of x[i + 1]): m, s, g"""
    def ends(inside, end):
        d = np.full(R, rnd(inside))
        d[0] = d[-1] = rnd(end)
        return d
    gd = np.zeros(R)
    gd[0], gd[-1] = -0.5, 0.5
    return ((ends(2.0 * h / 3.0, h / 3.0), rnd(h / 6.0), rnd(h / 6.0)), (ends(2.0 / h, 1.0 / h), rnd(-1.0 / h), rnd(-1.0 / h)),
            (gd, 0.5, -0.5))


def tri_abs(t):
    return np.abs(t[0]), abs(t[1]), abs(t[2])


def tri_apply(t, x, axis):
    """a tridiagonal 1-D matrix along one axis of a [R, R, R] array, by slicing"""
    d, below, above = t
    x = np.moveaxis(x, axis, 0)
    y = d[:, None, None] * x
    y[1:] += below * x[:-1]
    y[:-1] += above * x[1:]
    return np.moveaxis(y, 0, axis)


class FreeLevel:
    """Level without a Kronecker product: the same fields and methods (no A, A0, WtW), the 1-D matrices applied along one
    axis at a time, the screen term as lam W^T (W x).  dtype=np.float32 rounds what the device holds in float32 -- the 1-D
    coefficients, the weights, v, b, diag, u = W x and the result of apply -- to float32 after it is formed in float64: the
    device's stores, not its order of operations.  W64 keeps the float64 weights (the device's iso uses those)."""

    def __init__(self, points, normals, depth, point_weight=4.0, scale=1.1, dtype=np.float64):
        rnd = self.rnd = _f32 if dtype == np.float32 else _same
        lo, side = box(points, scale)
        self.lo, self.R, self.h = lo, 2 ** depth + 1, side / 2 ** depth
        R, h = self.R, self.h
        nrm = np.asarray(normals, np.float32).astype(np.float64)
        n = nrm.shape[0]
        self.W64, cell = weights(points, lo, h, R)
        self.W = self.W64.copy()
        self.W.data = rnd(self.W.data)
        self.Wt = self.W.T.tocsr()
        self.n_occ = int(np.unique(cell).size)
        self.a = self.n_occ * h * h / n
        self.lam = point_weight * self.a / h
        self.m, self.s, self.g = tri_1d(R, h, rnd)
        self.v = rnd((self.a / h ** 3) * (self.Wt @ (-nrm)))
        self.v_abs = (self.a / h ** 3) * (self.Wt @ np.abs(nrm))
        self.b = rnd(self._rhs(self.v, self.m, self.g))
        self.b_abs = self._rhs(self.v_abs, tri_abs(self.m), tri_abs(self.g))
        dm, ds = self.m[0], self.s[0]
        outer = lambda p, q, r: p[:, None, None] * q[None, :, None] * r[None, None, :]
        stencil = rnd(outer(ds, dm, dm) + outer(dm, ds, dm) + outer(dm, dm, ds)).reshape(-1)
        self.diag = rnd(stencil + self.lam * np.asarray(self.W.power(2).sum(axis=0)).reshape(-1))

    def _rhs(self, v, m, g):
        R = self.R
        vx, vy, vz = (v[:, a].reshape(R, R, R) for a in range(3))
        return (tri_apply(g, tri_apply(m, tri_apply(m, vx, 2), 1), 0) + tri_apply(m, tri_apply(g, tri_apply(m, vy, 2), 1), 0) +
                tri_apply(m, tri_apply(m, tri_apply(g, vz, 2), 1), 0)).reshape(-1)

    def _stencil(self, x, m, s):
        x = x.reshape(self.R, self.R, self.R)
        mz, sz = tri_apply(m, x, 2), tri_apply(s, x, 2)
        return (tri_apply(s, tri_apply(m, mz, 1), 0) + tri_apply(m, tri_apply(s, mz, 1) + tri_apply(m, sz, 1), 0)).reshape(-1)

    def apply(self, x):
        x = np.asarray(x, np.float64).reshape(-1)
        return self.rnd(self._stencil(x, self.m, self.s) + self.lam * (self.Wt @ self.rnd(self.W @ x)))

    def apply_abs(self, x):
        """the sum over the absolute values of the terms of A x"""
        ax = np.abs(np.asarray(x, np.float64).reshape(-1))
        return self._stencil(ax, tri_abs(self.m), tri_abs(self.s)) + self.lam * (self.Wt @ (self.W @ ax))


def prolong(xc, Rc, odd_weight=0.5):
    """prolong_matrix(Rc) @ xc without the matrix.  odd_weight is the weight of each of the two coarse neighbours of an odd
    node along one axis: 0.5 is the definition, another value is a deliberately wrong prolongation for checking that a
    test would notice one."""
    x = np.asarray(xc, np.float64).reshape(Rc, Rc, Rc)
    for axis in range(3):
        x = np.moveaxis(x, axis, 0)
        y = np.empty((2 * x.shape[0] - 1,) + x.shape[1:])
        y[0::2] = x
        y[1::2] = odd_weight * (x[:-1] + x[1:])
        x = np.moveaxis(y, 0, axis)
    return x.reshape(-1)


def one_step_cascade(points, normals, depth, dtype=np.float64, point_weight=4.0, scale=1.1, odd_weight=0.5):
    """(x of the finest level, its FreeLevel): per level 3 .. depth exactly one Jacobi-preconditioned CG step from x0 = 0 or
    the prolongation of the level below: r = b - A x0, z = r / diag, alpha = r.z / z.A z, x = x0 + alpha z.
    dtype=np.float64 is the yardstick; dtype=np.float32 rounds every stored vector (x, r, p = z, A p, u), alpha and what
    FreeLevel rounds to float32 after each step; the dot products stay float64, as on the device."""
    rnd = _f32 if dtype == np.float32 else _same
    x, lev = None, None
    for d in range(MIN_DEPTH, depth + 1):
        lev = FreeLevel(points, normals, d, point_weight, scale, dtype)
        x0 = np.zeros(lev.R ** 3) if x is None else rnd(prolong(x, (lev.R + 1) // 2, odd_weight))
        r = rnd(lev.b - lev.apply(x0))
        p = rnd(r / lev.diag)
        ap = lev.apply(p)
        alpha = rnd(np.dot(r, p) / np.dot(p, ap))
        x = rnd(x0 + alpha * p)
    return x, lev


def piece_cases():
    """name -> (points, normals, scale): the inputs of the node-by-node comparisons of one level"""
    rng = np.random.default_rng(5)
    unit = np.array([[0.0, 0.6, 0.8]], np.float32)
    corners = np.array([[0, 0, 0], [1, 1, 1]], np.float32)
    out = {}
    # one point inside a cell; two points without normals span the box
    out['inside'] = (np.concatenate([np.array([[0.30, 0.41, 0.52]], np.float32), corners]),
                     np.concatenate([unit, np.zeros((2, 3), np.float32)]), 1.1)
    # one point exactly on a node of both depths; scale 1.0 puts the corner points on the last node (the clamp, t = 1)
    out['on_node_scale1'] = (np.concatenate([np.array([[0.5, 0.25, 0.75]], np.float32), corners]),
                             np.concatenate([unit, np.array([[1, 0, 0], [0, -2, 0.5]], np.float32)]), 1.0)
    # 300 identical points in one cell and 5 elsewhere: the ends of the cell sort's segments
    few = rng.random((5, 3)).astype(np.float32)
    out['dense_cell'] = (np.concatenate([np.repeat(np.array([[0.61, 0.33, 0.47]], np.float32), 300, 0), few, corners]),
                         np.concatenate([np.repeat(unit, 300, 0), rng.standard_normal((5, 3)).astype(np.float32),
                                         np.zeros((2, 3), np.float32)]), 1.1)
    out['sphere'] = sphere(2000, 3) + (1.1,)
    # normals of length 0 for half of the points; scale 1.0: the extreme points of a real cloud on the last node
    pts, nrm = sphere(2000, 4)
    nrm = nrm.copy()
    nrm[::2] = 0.0
    out['half_zero_scale1'] = (pts, nrm, 1.0)
    return out


def prolong_matrix(Rc):
    Rf = 2 * Rc - 1
    rows, cols, vals = [], [], []
    for i in range(Rf):
        if i % 2 == 0:
            rows.append(i), cols.append(i // 2), vals.append(1.0)
        else:
            rows += [i, i]
            cols += [i // 2, i // 2 + 1]
            vals += [0.5, 0.5]
    P = sp.csr_matrix((vals, (rows, cols)), shape=(Rf, Rc))
    return kron3(P, P, P)


def solve(points, normals, depth, point_weight=4.0, scale=1.1, tol=1e-12):
    """the cascade: (chi of the finest level, its Level, iterations per level)"""
    x, iters, lev = None, [], None
    for d in range(MIN_DEPTH, depth + 1):
        lev = Level(points, normals, d, point_weight, scale)
        x0 = np.zeros(lev.R ** 3) if x is None else prolong_matrix((lev.R + 1) // 2) @ x
        count = [0]
        M = sp.diags(1.0 / lev.diag)
        x, info = spl.cg(lev.A, lev.b, x0=x0, rtol=tol, atol=0.0, M=M, maxiter=20000, callback=lambda _: count.__setitem__(0, count[0] + 1))
        assert info == 0
        iters.append(count[0])
    return x, lev, iters


def iso_value(lev, chi):
    return float(np.mean(lev.W @ np.asarray(chi, np.float64).reshape(-1)))


def volume(lev, chi):
    """(float32 [R, R, R] volume with the border rule, iso)"""
    iso = iso_value(lev, chi)
    R = lev.R
    vol = (np.asarray(chi, np.float64).reshape(R, R, R) - iso).astype(np.float32)
    border = border_mask(R)
    vol[border] = -np.abs(vol[border])
    return vol, iso


def border_mask(R):
    m = np.zeros((R, R, R), bool)
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True, True, True
    return m


def trilinear(vol, R, g):
    """the trilinear interpolant of a [R, R, R] grid at grid coordinates g [n, 3]"""
    c = np.clip(np.floor(g), 0, R - 2).astype(np.int64)
    t = g - c
    out = np.zeros(g.shape[0])
    for k in range(8):
        kx, ky, kz = k >> 2, (k >> 1) & 1, k & 1
        w = (t[:, 0] if kx else 1.0 - t[:, 0]) * (t[:, 1] if ky else 1.0 - t[:, 1]) * (t[:, 2] if kz else 1.0 - t[:, 2])
        out += w * vol[c[:, 0] + kx, c[:, 1] + ky, c[:, 2] + kz]
    return out


def ray_crossings(vol, lo, h, R, origin, dirs, r_max, steps=400):
    """the first radius along each ray origin + r dir at which the interpolated volume turns from > 0 to <= 0 (NaN: none)"""
    rs = np.linspace(0.0, r_max, steps + 1)
    vals = np.stack([trilinear(np.asarray(vol, np.float64), R, (origin + r * dirs - lo) / h) for r in rs])
    out = np.full(dirs.shape[0], np.nan)
    for j in range(dirs.shape[0]):
        col = vals[:, j]
        k = np.nonzero((col[:-1] > 0) & (col[1:] <= 0))[0]
        if k.size:
            a, b = col[k[0]], col[k[0] + 1]
            out[j] = rs[k[0]] + (rs[k[0] + 1] - rs[k[0]]) * a / (a - b)
    return out


def sphere(n=20000, seed=0, radius=0.5):
    """n points on a sphere: normalised Gaussians of default_rng(seed); normals = directions"""
    u = np.random.default_rng(seed).standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (radius * u).astype(np.float32), u.astype(np.float32)
