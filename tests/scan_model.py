"""Float64 numpy model of the ray-casting kernels (points2surf_amd/csrc/p2s_meshray.inl; the octree walk's
helpers: p2s_mesh_octree.inl): the same operations in the same
association, contraction off, so the device's t is expected to equal the model's bit for bit.

* ``cast``: brute force, every ray against every triangle (Moeller-Trumbore through the face's own cross product:
  u = -(e2 . q) / dn, v = (e1 . q) / dn, t = -(s . n) / dn with n = e1 x e2, s = o - a, q = s x d, dn = d . n); the
  smallest t in (0, t_max] wins, ties go to the smallest face id, both sides are hit, a degenerate face (2^-90 rule) and
  a ray in the face's plane miss, a hit whose computed point lies more than E = 2^-24 max(|mesh|, |o|) outside the face's
  bounding box is discarded, a direction component below 2^-1022 counts as 0, a non-finite or zero ray
  misses (face -1, t = inf).  Reports the runner-up t per ray
  (``second``: the smallest t over the OTHER faces), as mesh_sdf_model reports ``second``.
* ``rotation`` / ``scan_rays``: the sensor frame of DESIGN 4.8 f6 (camera at the origin looking along +y, x right, z up,
  object at R(q) p + location) and the rays in model space, in the order (scan, row j, column i).
* ``tof_scan``: cast, stable compaction of the hits in ray order, p = o + t d, p_noisy = o + (t + sigma g) d.
* ``sample_surface`` / ``query_points``: trimesh's area-weighted surface samples and the query points of
  source/sdf.py:288-315 with every deviate from one RandomState: samples, offsets, far points.
"""
import numpy as np

from mesh_sdf_model import DEGENERATE_REL, cross3, dot3

RAY_BOX_REL = 2.0 ** -24
BIG = 1.0e300
TINY = 2.2250738585072014e-308          # the smallest normal float64


def triangles(verts, faces):
    """[F, 9] float64: a, b, c of every face"""
    v = np.asarray(verts, np.float64)
    return v[np.asarray(faces)].reshape(-1, 9)


def tri_prep(T):
    A, B, C = T[:, 0:3], T[:, 3:6], T[:, 6:9]
    e1, e2 = B - A, C - A
    n = cross3(e1, e2)
    ok = dot3(n, n) > DEGENERATE_REL * (dot3(e1, e1) * dot3(e2, e2))
    lo = np.minimum(A, np.minimum(B, C))
    hi = np.maximum(A, np.maximum(B, C))
    return A, e1, e2, n, lo, hi, ok


def face_normals(T):
    """the handle's stored normals: n * (1 / sqrt(n . n)), 0 for a degenerate face"""
    _, _, _, n, _, _, ok = tri_prep(T)
    with np.errstate(all='ignore'):
        inv = 1.0 / np.sqrt(dot3(n, n))
        return np.where(ok[:, None], n * inv[:, None], 0.0)


def mesh_scale(T):
    return float(np.abs(T).max())


def ray_valid(o, d):
    with np.errstate(invalid='ignore'):
        fin = (np.abs(o) <= BIG).all(1) & (np.abs(d) <= BIG).all(1)
    return fin & (d != 0.0).any(1)


def hit_table(T, rays, t_max=np.inf, scale=None, box_rule=True):
    """[n, F] t of every (ray, face) pair, inf where the pair does not hit (``box_rule=False``: without the discard of
    hits outside the face's bounding box, to show what the rule removes)"""
    rays = np.array(rays, np.float64)
    rays[:, 3:6][np.abs(rays[:, 3:6]) < TINY] = 0.0                  # subnormal direction components count as 0
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    A, e1, e2, n, lo, hi, ok = (x[None] for x in tri_prep(T))
    scale = mesh_scale(T) if scale is None else scale
    with np.errstate(all='ignore'):
        E = (np.maximum(scale, np.abs(rays[:, 0:3]).max(1)) * RAY_BOX_REL)[:, None, None]
        dn = dot3(d, n)
        s = o - A
        q = cross3(s, np.broadcast_to(d, s.shape))
        u, v, t = -dot3(e2, q) / dn, dot3(e1, q) / dn, -dot3(s, n) / dn
        hit = ok & (dn != 0.0) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t > 0.0) & (t <= t_max)
        x = o + t[..., None] * d
        if box_rule:
            hit &= ((x >= lo - E) & (x <= hi + E)).all(-1)
    hit &= (ray_valid(rays[:, 0:3], rays[:, 3:6]) & (t_max > 0.0))[:, None]
    return np.where(hit, t, np.inf)


def cast(T, rays, t_max=np.inf, scale=None, chunk=None):
    """(t [n], face [n], second [n]): first hit, its face (-1: miss), the smallest t over the other faces"""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    n, F = len(rays), len(T)
    scale = mesh_scale(T) if scale is None else scale
    chunk = chunk or max(1, int(1.5e6 // max(F, 1)))
    t_out, f_out, s_out = np.full(n, np.inf), np.full(n, -1, np.int64), np.full(n, np.inf)
    for a in range(0, n, chunk):
        tab = hit_table(T, rays[a:a + chunk], t_max, scale)
        f = tab.argmin(1)                                  # the first of equal minima: the smallest face id
        idx = np.arange(len(tab))
        t = tab[idx, f]
        tab[idx, f] = np.inf
        t_out[a:a + chunk], s_out[a:a + chunk] = t, tab.min(1)
        f_out[a:a + chunk] = np.where(t < np.inf, f, -1)
    return t_out, f_out, s_out


def rotation(q):
    """R(q) of a unit quaternion (w, x, y, z), in the association of p2s_mesh_tof_scan"""
    w, x, y, z = (float(c) for c in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def scan_rays(locations, rotations, W, H, tan_w, tan_h):
    """[S * H * W, 6]: origin R^T (-location), direction R^T dir of pixel (i, j), ray = (scan * H + j) * W + i"""
    i, j = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    sx = ((i + 0.5) - 0.5 * W) * ((2.0 * tan_w) / W)
    sz = ((j + 0.5) - 0.5 * H) * ((2.0 * tan_h) / H)
    SX, SZ = np.broadcast_to(sx[None, :], (H, W)), np.broadcast_to(sz[:, None], (H, W))
    ln = np.sqrt((SX * SX + 1.0) + SZ * SZ)
    c = np.stack([SX / ln, 1.0 / ln, SZ / ln], -1).reshape(-1, 3)
    out = []
    for loc, q in zip(np.asarray(locations, np.float64), np.asarray(rotations, np.float64)):
        R = rotation(q)
        o = (R[0] * -loc[0] + R[1] * -loc[1]) + R[2] * -loc[2]
        d = (R[0][None, :] * c[:, 0:1] + R[1][None, :] * c[:, 1:2]) + R[2][None, :] * c[:, 2:3]
        out.append(np.concatenate([np.broadcast_to(o, d.shape), d], 1))
    return np.concatenate(out) if out else np.zeros((0, 6))


def tof_scan(T, locations, rotations, sigma, noise, W, H, tan_w, tan_h, max_distance):
    rays = scan_rays(locations, rotations, W, H, tan_w, tan_h)
    rays[:, 3:6][np.abs(rays[:, 3:6]) < TINY] = 0.0
    t, face, second = cast(T, rays, max_distance)
    hit = face >= 0
    o, d, th = rays[hit, 0:3], rays[hit, 3:6], t[hit]
    tn = th + sigma * np.asarray(noise, np.float64).reshape(-1)[hit]
    return dict(rays=rays, t=t, face_all=face, second=second, hits_per_scan=hit.reshape(len(locations), -1).sum(1).astype(np.int32),
                points_noisefree=o + th[:, None] * d, points=o + tn[:, None] * d, face=face[hit], normals=face_normals(T)[face[hit]])


def sample_surface(verts, faces, count, rng):
    """trimesh.sample.sample_surface: ``count`` face picks (searchsorted on the cumulative areas), then (count, 2)
    folded barycentric lengths -> (points [count, 3] float64, face ids)"""
    tri = np.asarray(verts, np.float64)[np.asarray(faces)]
    area = np.sqrt((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(1)) / 2.0
    cum = np.cumsum(area)
    idx = np.minimum(np.searchsorted(cum, rng.random_sample(count) * cum[-1]), len(cum) - 1)
    ln = rng.random_sample((count, 2, 1))
    fold = ln.sum(1).reshape(-1) > 1.0
    ln[fold] -= 1.0
    ln = np.abs(ln)
    vec = tri[idx, 1:] - tri[idx, 0][:, None, :]
    return tri[idx, 0] + (vec * ln).sum(1), idx


def query_points_from(samples, face, fn, u_off, u_far, patch_radius):
    """the construction alone: far points u - 1/2 in front, then samples + ((u - 1/2) 2 r) n_face; float32"""
    off = ((np.asarray(u_off, np.float64) - 0.5) * 2.0) * patch_radius
    close = np.asarray(samples, np.float32).astype(np.float64) + off[:, None] * fn[np.asarray(face)]
    far = np.asarray(u_far, np.float64).reshape(-1, 3) - 0.5
    return np.concatenate([far, close]).astype(np.float32), off


def query_points(verts, faces, seed, num=2000, patch_radius=4.0 / 256, far_ratio=0.1):
    """(points float32 [num, 3], samples, face ids, offsets): every deviate from RandomState(seed) in the order surface
    samples, offsets, far points"""
    n_far = int(num * far_ratio)
    n_close = num - n_far
    rng = np.random.RandomState(seed)
    samples, face = sample_surface(verts, faces, n_close, rng)
    u_off = rng.random_sample(n_close)
    u_far = rng.random_sample(3 * n_far)
    pts, off = query_points_from(samples.astype(np.float32), face, face_normals(triangles(verts, faces)), u_off, u_far, patch_radius)
    return pts, samples, face, off
