"""float64 numpy model of points2surf_amd.prepare: the same operations in the same order -- the order
statistics by bisection on the ordered bit pattern, the outlier statistic over a brute-force n^2 search with the id
tie-break and ``math.fsum`` for mean and std, the voxel winner per cell, the unit cube -- so that ids, bounds, d_i, R and the
normalised bytes of the device must equal these.

Also the seeded clouds that the CPU and the GPU tests share.
"""
import math

import numpy as np


def _f32(points):
    return np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))


def finite_ids(points):
    return np.nonzero(np.isfinite(_f32(points)).all(axis=1))[0].astype(np.int32)


# ---- crop ---------------------------------------------------------------------------------------------------------------

def ordered_key(x):
    """uint32 keys in the order of the float32 values; -0 counts as +0"""
    b = (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def from_key(k):
    k = np.uint32(k)
    b = (k & np.uint32(0x7fffffff)) if (k & np.uint32(0x80000000)) else ~k
    return np.array([b], np.uint32).view(np.float32)[0]


def order_statistic(x, rank):
    """the value of rank ``rank`` (0-based) of the float32 array x: the smallest key K with count(key <= K) > rank, built bit
    by bit from the top -- 32 counting passes, as the device does"""
    key = ordered_key(x)
    K = 0
    for bit in range(31, -1, -1):
        T = K | (1 << bit)
        if int((key < np.uint32(T)).sum()) <= rank:
            K = T
    return from_key(K)


def quantile_ranks(n, q):
    return int(math.floor(q * (n - 1))), int(math.ceil((1.0 - q) * (n - 1)))


def crop(points, quantile=0.01, margin=1.0):
    """(kept ids int32, bounds float64 [12]: lo[3], hi[3] order statistics, widened box lo[3], hi[3])"""
    p = _f32(points)
    n = p.shape[0]
    if quantile == 0 or n == 0:
        return np.arange(n, dtype=np.int32), np.zeros(12)
    r_lo, r_hi = quantile_ranks(n, quantile)
    lo = np.array([order_statistic(p[:, a], r_lo) for a in range(3)], np.float64)
    hi = np.array([order_statistic(p[:, a], r_hi) for a in range(3)], np.float64)
    w = margin * (hi - lo)
    blo, bhi = lo - w, hi + w
    x = p.astype(np.float64)
    keep = ((x >= blo) & (x <= bhi)).all(axis=1)
    return np.nonzero(keep)[0].astype(np.int32), np.concatenate([lo, hi, blo, bhi])


# ---- statistical outliers -----------------------------------------------------------------------------------------------

def outlier_statistic(points, k, chunk=256):
    """d [n] float64: (sum of the distances to the k + 1 nearest cloud points, the point itself included, added in ascending
    (distance, id) order) / k; k clamped to n - 1"""
    p = _f32(points).astype(np.float64)
    n = p.shape[0]
    k = min(int(k), n - 1)
    out = np.empty(n, np.float64)
    for a in range(0, n, chunk):
        d = p[None, :, :] - p[a:a + chunk, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.argsort(d2, axis=1, kind='stable')[:, :k + 1]                 # stable: equal distances stay in id order
        dist = np.sqrt(np.take_along_axis(d2, order, axis=1))
        out[a:a + chunk] = np.cumsum(dist, axis=1)[:, -1] / float(k)             # cumsum adds one after the other
    return out


def outlier_threshold(d, std_ratio):
    n = len(d)
    mean = math.fsum(d) / n
    std = math.sqrt(math.fsum((d - mean) * (d - mean)) / n)
    return mean, std, mean + std_ratio * std


def remove_outliers(points, k=16, std_ratio=2.0):
    """(kept ids, info): info d, mean, std, threshold, k -- all None / 0 where the stage is off or n < 2"""
    p = _f32(points)
    n = p.shape[0]
    if std_ratio == 0 or n < 2:
        return np.arange(n, dtype=np.int32), dict(d=None, mean=0.0, std=0.0, threshold=0.0, k=0)
    d = outlier_statistic(p, k)
    mean, std, thr = outlier_threshold(d, std_ratio)
    return np.nonzero(d <= thr)[0].astype(np.int32), dict(d=d, mean=mean, std=std, threshold=thr, k=min(int(k), n - 1))


# ---- thinning -----------------------------------------------------------------------------------------------------------

def random_ids(n, max_points, seed):
    """the reference's rule with a seed: the ids in the order drawn"""
    return np.random.RandomState(int(seed)).choice(int(n), int(max_points), replace=False).astype(np.int32)


def _box(p):
    return p.min(axis=0).astype(np.float64) + 0.0, p.max(axis=0).astype(np.float64) + 0.0      # -0 counts as +0


def voxel_cells(points, R):
    """(linear cell id int64 [n], squared distance to the cell's centre float64 [n])"""
    p = _f32(points)
    lo, hi = _box(p)
    ext = float((hi - lo).max())
    scale = float(R) / ext if ext > 0.0 else 0.0
    cell = ext / float(R)
    x = p.astype(np.float64)
    ia = np.minimum(np.floor((x - lo) * scale), float(R - 1)).astype(np.int64)
    c = lo + (ia.astype(np.float64) + 0.5) * cell
    d = x - c
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return (ia[:, 0] * R + ia[:, 1]) * R + ia[:, 2], d2


def occupied(points, R):
    return int(np.unique(voxel_cells(points, R)[0]).size)


def search_resolution(points, max_points, count=None):
    """the definition of R (count(R) is not monotone over grids that do not nest)"""
    count = count or (lambda R: occupied(points, R))
    lo, hi = 1, 1024
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if count(mid) <= max_points:
            lo = mid
        else:
            hi = mid - 1
    return lo


def voxel_thin(points, max_points=None, resolution=None):
    """(kept ids in input order, R (0: nothing to do), occupied cells)"""
    p = _f32(points)
    n = p.shape[0]
    if n == 0 or (resolution is None and n <= max_points):
        return np.arange(n, dtype=np.int32), 0, 0
    R = int(resolution) if resolution is not None else search_resolution(p, max_points)
    lin, d2 = voxel_cells(p, R)
    order = np.lexsort((np.arange(n), d2, lin))                                  # by cell, then distance, then id
    first = np.ones(n, bool)
    first[1:] = lin[order][1:] != lin[order][:-1]
    kept = np.sort(order[first]).astype(np.int32)
    return kept, R, int(kept.size)


# ---- unit cube ----------------------------------------------------------------------------------------------------------

def normalize(points):
    """(float32 [n, 3], centre float64 [3], scale float64); ValueError('extent 0') for a cloud of coincident points"""
    p = _f32(points)
    lo, hi = _box(p)
    ext = float((hi - lo).max())
    if not ext > 0.0:
        raise ValueError('extent 0')
    c = (lo + hi) * 0.5
    s = 1.0 / ext
    return ((p.astype(np.float64) - c) * s).astype(np.float32), c, s


def restore(vertices, centre, scale):
    return np.asarray(vertices, np.float32).astype(np.float64) / float(scale) + np.asarray(centre, np.float64)


# ---- the stages composed ------------------------------------------------------------------------------------------------

def prepare(points, crop_quantile=0.01, crop_margin=1.0, k=16, std_ratio=2.0, max_points=150000, thin='random', seed=42):
    """(points float32 [m, 3], kept ids int32 [m] into the input, (centre, scale), report)"""
    p = _f32(points)
    rep = dict(points_in=int(p.shape[0]))
    kept = finite_ids(p)
    rep['nonfinite'] = rep['points_in'] - kept.size
    ids, bounds = crop(p[kept], crop_quantile, crop_margin)
    rep['cropped'] = kept.size - ids.size
    kept = kept[ids]
    ids, info = remove_outliers(p[kept], k, std_ratio)
    rep['outliers'] = kept.size - ids.size
    rep.update(mean=info['mean'], std=info['std'], threshold=info['threshold'])
    kept = kept[ids]
    rep['R'] = 0
    before = kept.size
    if max_points and kept.size > max_points:
        if thin == 'random':
            ids = random_ids(kept.size, max_points, seed)
        else:
            ids, rep['R'], _ = voxel_thin(p[kept], max_points)
        kept = kept[ids]
    rep['thinned'] = before - kept.size
    out, c, s = normalize(p[kept])
    rep['points_out'] = int(kept.size)
    return out, kept.astype(np.int32), (c, s), rep


# ---- clouds -------------------------------------------------------------------------------------------------------------

SIZES = (1, 2, 17, 257, 4099)


def seeded_cloud(n, seed=0):
    """a blob of both signs with a few coordinates exactly +-0 and repeated values"""
    rng = np.random.default_rng(1000 * seed + n)
    p = (0.3 * rng.standard_normal((n, 3)) + np.array([0.05, -0.1, 0.2])).astype(np.float32)
    if n >= 17:
        p[3, 0] = 0.0
        p[5, 0] = -0.0
        p[7] = p[11]                                 # an exact duplicate
        p[2, 1] = p[9, 1]                            # a repeated coordinate
    return p


def scan_like(n, seed=0, outliers=0.005, far=0):
    """a noisy sphere shell of n points with a fraction of uniform outliers in a box 3 times its size and ``far`` returns
    at 100 times the extent"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    p = 0.5 * v / np.linalg.norm(v, axis=1, keepdims=True) + 0.002 * rng.standard_normal((n, 3))
    m = int(round(outliers * n))
    if m:
        p[rng.permutation(n)[:m]] = rng.uniform(-1.5, 1.5, (m, 3))
    if far:
        p[rng.permutation(n)[:far]] = 100.0 * rng.choice([-1.0, 1.0], (far, 3)) * rng.uniform(0.5, 1.0, (far, 3))
    return p.astype(np.float32)
