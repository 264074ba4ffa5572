"""numpy float64 model of the winding-number kernels (points2surf_amd/csrc/p2s_meshdist.hip: winding_term,
p2s_md_winding_kernel, p2s_md_wtree_kernel; the moments: p2s_meshbuild.inl; the walk's helpers: p2s_mesh_octree.inl):
the exact generalised winding number (Jacobson et al. 2013, with the solid angle of van Oosterom & Strackee 1983), the moments of a set of triangles, the dipole that stands for them and the bound on
its error.  No device."""
import numpy as np

DEGENERATE_REL = 2.0 ** -90


def _dot(a, b):
    return (a * b).sum(-1)


def _terms(a, b, c):
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    num = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    return num, den, la * lb * lc


def winding_terms(tris, q, refine=True):
    """atan2 term (half the signed solid angle) of every triangle ``tris`` [F, 3, 3] seen from every query ``q`` [n, 3]:
    [n, F].  The corners minus the query are exact in float64 for float32 data, but numerator and denominator both cancel
    when the query lies next to the line of an edge, between its ends: with ``refine`` the terms where both are below 2^-10
    |a||b||c| are recomputed in numpy's longdouble (80-bit on x86; where longdouble is float64 they stay as they are)."""
    a = tris[None, :, 0] - q[:, None]
    b = tris[None, :, 1] - q[:, None]
    c = tris[None, :, 2] - q[:, None]
    num, den, scale = _terms(a, b, c)
    out = np.arctan2(num, den)
    if refine:
        ill = np.abs(num) + np.abs(den) < 2.0 ** -10 * scale
        if ill.any():
            L = np.longdouble
            num, den, _ = _terms(a[ill].astype(L), b[ill].astype(L), c[ill].astype(L))
            out[ill] = np.arctan2(num, den).astype(np.float64)
    return out


def winding_exact(verts, faces, q, chunk=64, workers=4):
    """w(p) = sum over the faces of the solid angle / 4 pi, for every query [n]"""
    from concurrent.futures import ThreadPoolExecutor
    tris = np.asarray(verts, np.float64)[np.asarray(faces)]
    q = np.asarray(q, np.float64)
    out = np.empty(len(q))

    def run(i):
        out[i:i + chunk] = winding_terms(tris, q[i:i + chunk]).sum(1) / (2.0 * np.pi)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(run, range(0, len(q), chunk)))
    return out


def moments(tris):
    """N = sum 1/2 (b - a) x (c - a) [3] and A = sum 1/2 |(b - a) x (c - a)|; a face with
    |ab x ac|^2 <= 2^-90 |ab|^2 |ac|^2 adds 0 to both.  Also the number of such faces."""
    ab, ac = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    n = np.cross(ab, ac)
    ok = _dot(n, n) > DEGENERATE_REL * (_dot(ab, ab) * _dot(ac, ac))
    return 0.5 * n[ok].sum(0), 0.5 * np.sqrt(_dot(n[ok], n[ok])).sum(), int((~ok).sum())


def box_of(tris):
    """centre and half-diagonal of the axis-aligned box of whole triangles"""
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    return 0.5 * (lo + hi), 0.5 * np.sqrt(((hi - lo) ** 2).sum())


def node_bound(area, r, d):
    """|exact - dipole| <= A r / (2 pi (d - r)^3) for d > r: the kernel K(x) = n . (x - p) / (4 pi |x - p|^3) has
    |grad K| <= 1 / (2 pi |x - p|^3), every point of the box lies within r of its centre and at least d - r from p"""
    return area * r / (2.0 * np.pi * (d - r) ** 3)


def cluster(tris, c, r, p):
    """for the triangles ``tris`` [T, 3, 3] inside the box (centre ``c``, half-diagonal ``r``) and the query ``p``:
    the exact sum of their winding terms, the dipole N . (c - p) / (4 pi d^3) and the bound on their difference"""
    N, A, _ = moments(tris)
    cp = np.asarray(c, np.float64) - np.asarray(p, np.float64)
    d = np.sqrt(_dot(cp, cp))
    exact = winding_terms(tris, np.asarray(p, np.float64)[None])[0].sum() / (2.0 * np.pi)
    return exact, _dot(N, cp) / (4.0 * np.pi * d ** 3), node_bound(A, r, d)


def rounding(n_faces, terms, n_degenerate=0):
    """the rounding term of the device's bound: 2^-53 F (K + F / 256 + 32) + D 2^-46 / pi"""
    return 2.0 ** -53 * n_faces * (terms + n_faces / 256.0 + 32.0) + n_degenerate * 2.0 ** -46 / np.pi
