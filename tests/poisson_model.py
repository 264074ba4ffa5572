"""float64 restatement of the Screened Poisson baseline (include/p2s_hip.h) with scipy.sparse: the box,
the levels, W, the 1-D matrices, A and b as Kronecker products, the cascade solved to 1e-12, iso, the volume with its
border rule.  The yardstick of points2surf_amd/csrc/p2s_poisson.hip; also the sums over absolute values that bound the
rounding of the device's float32 pieces."""
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
