"""The numpy model of points2surf_amd.prepare (tests/prepare_model.py) against numpy itself and hand-made cases (no device)."""
import math

import numpy as np
import pytest

import prepare_model as M


@pytest.mark.parametrize('seed,n,N', [(42, 1000, 150), (7, 151, 150), (0, 5, 5)])
def test_random_rule_is_numpys_choice(seed, n, N):
    ids = M.random_ids(n, N, seed)
    assert ids.dtype == np.int32
    assert np.array_equal(ids, np.random.RandomState(seed).choice(n, N, replace=False))
    assert np.unique(ids).size == N
    assert np.array_equal(ids, M.random_ids(n, N, seed))


def test_ordered_key_orders_like_the_values():
    x = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    k = M.ordered_key(x).astype(np.int64)
    assert k[3] == k[4]                              # -0 counts as +0
    assert (np.diff(np.delete(k, 3)) > 0).all()
    for v in x:
        assert M.from_key(M.ordered_key(np.array([v], np.float32))[0]) == v


@pytest.mark.parametrize('n', M.SIZES)
@pytest.mark.parametrize('q', (0.01, 0.1, 0.49))
def test_quantile_ranks_equal_sorted(n, q):
    p = M.seeded_cloud(n, seed=3)
    r_lo, r_hi = M.quantile_ranks(n, q)
    assert 0 <= r_lo <= r_hi <= n - 1
    for a in range(3):
        s = np.sort(p[:, a])
        assert M.order_statistic(p[:, a], r_lo) == s[r_lo]
        assert M.order_statistic(p[:, a], r_hi) == s[r_hi]
    ids, b = M.crop(p, q, 0.0)
    x = p.astype(np.float64)
    inside = ((x >= b[0:3]) & (x <= b[3:6])).all(axis=1)
    assert np.array_equal(ids, np.nonzero(inside)[0])


def test_order_statistic_negative_values_zeros_and_repeats():
    x = np.array([-2.0, -2.0, -0.0, 0.0, 0.0, -1.0, 3.0, -2.0, 3.0, -5.0], np.float32)
    s = np.sort(x)
    for r in range(len(x)):
        assert M.order_statistic(x, r) == s[r]


def test_crop_removes_the_stray_only():
    p = M.scan_like(2000, seed=1, outliers=0.0)
    p[17] = (250.0, -3.0, 0.1)
    ids, _ = M.crop(p, 0.01, 1.0)
    assert np.array_equal(ids, np.delete(np.arange(2000), 17))
    ids, b = M.crop(p, 0.0, 1.0)
    assert np.array_equal(ids, np.arange(2000)) and not b.any()


def test_outlier_statistic_by_hand():
    # four points on a line at 0, 1, 3, 7; k = 2: the two nearest others
    p = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0]], np.float32)
    d = M.outlier_statistic(p, 2)
    assert np.array_equal(d, np.array([(1 + 3) / 2, (1 + 2) / 2, (2 + 3) / 2, (4 + 6) / 2]))
    assert np.array_equal(M.outlier_statistic(p, 64), M.outlier_statistic(p, 3))        # k is clamped to n - 1
    mean, std, thr = M.outlier_threshold(d, 1.0)
    # d = 2, 1.5, 2.5, 5: mean 11 / 4, squared deviations 0.5625 + 1.5625 + 0.0625 + 5.0625 = 7.25
    assert mean == 2.75 and std == math.sqrt(7.25 / 4) and thr == mean + std
    ids, info = M.remove_outliers(p, 2, 1.0)
    assert np.array_equal(ids, [0, 1, 2]) and info['k'] == 2


def test_outliers_duplicates_and_equal_points():
    k = 4
    rng = np.random.default_rng(5)
    p = np.concatenate([np.repeat(np.array([[0.25, -0.5, 0.125]], np.float32), k + 2, 0), rng.uniform(-1, 1, (60, 3)).astype(np.float32)])
    d = M.outlier_statistic(p, k)
    assert (d[:k + 2] == 0.0).all() and (d[k + 2:] > 0.0).all()
    same = np.repeat(np.array([[1.5, 2.5, -3.5]], np.float32), 9, 0)
    ids, info = M.remove_outliers(same, k, 2.0)
    assert info['std'] == 0.0 and info['mean'] == 0.0 and np.array_equal(ids, np.arange(9))
    ids, info = M.remove_outliers(same[:1], k, 2.0)
    assert np.array_equal(ids, [0]) and info['d'] is None


def test_resolution_search_terminates_within_the_budget():
    p = M.scan_like(3000, seed=2)
    for N in (1, 2, 50, 700, 2999):
        R = M.search_resolution(p, N)
        assert 1 <= R <= 1024 and M.occupied(p, R) <= N
        ids, R2, occ = M.voxel_thin(p, N)
        assert R2 == R and occ == ids.size == M.occupied(p, R) and (np.diff(ids) > 0).all()
    assert M.search_resolution(p, 1) == 1
    ids, R, occ = M.voxel_thin(p, 3000)
    assert R == 0 and np.array_equal(ids, np.arange(3000))


def test_resolution_search_follows_the_definition_where_counts_are_not_monotone():
    calls = []

    def count(R):                                    # 600 cells at R = 512 although R = 300 .. 511 stay within the budget
        calls.append(R)
        return 600 if R == 512 else (R if R < 512 else 10 ** 6)

    assert M.search_resolution(None, 500, count) == 500
    assert calls[0] == 513 and len(calls) == 10      # ten halvings of 1 .. 1024


def test_voxel_by_hand():
    # the corners of the unit cube and points near them: R = 2 has 8 cells of edge 0.5 with centres at 0.25 / 0.75
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    inner = 0.25 + 0.5 * corners                     # exactly the centres
    p = np.concatenate([corners, inner])
    # R = 4: 0.75 * 4 = 3 is a face, so (0.75, 0.75, 0.75) shares the last cell with the clamped corner (1, 1, 1): 15 cells
    assert M.occupied(p, 1) == 1 and M.occupied(p, 2) == 8 and M.occupied(p, 4) == 15 and M.occupied(p, 5) == 16
    assert M.search_resolution(p, 8) == 3            # R = 3 puts every corner and its centre point together
    ids, R, occ = M.voxel_thin(p, 8)
    assert R == 3 and occ == 8
    ids2, _, _ = M.voxel_thin(p, resolution=2)
    assert np.array_equal(ids2, np.arange(8, 16))    # the centres win
    # a face point belongs to the upper cell, the box's upper face to the last cell; of a mirror pair the lower id stays
    q = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.25], [0.625, 0.25, 0.25], [0.875, 0.25, 0.25]], np.float32)
    lin, d2 = M.voxel_cells(q, 2)
    assert list(lin) == [0, 7, 4, 4, 4] and d2[3] == d2[4]
    assert list(M.voxel_thin(q, resolution=2)[0]) == [0, 1, 3]


@pytest.mark.parametrize('n', (2, 17, 257, 4099))
def test_normalize_then_restore(n):
    p = (M.seeded_cloud(n, seed=4).astype(np.float64) * 37.0 + np.array([120.0, -45.0, 8.0])).astype(np.float32)
    out, c, s = M.normalize(p)
    assert out.dtype == np.float32
    ext = (p.max(0).astype(np.float64) - p.min(0).astype(np.float64)).max()
    a = int(np.argmax(p.max(0).astype(np.float64) - p.min(0).astype(np.float64)))
    assert out[:, a].min() == -0.5 and out[:, a].max() == 0.5 and np.abs(out).max() <= 0.5
    back = M.restore(out, c, s)
    # the float32 rounding of a value of magnitude <= 0.5 is at most 2^-25, times the extent; float64 noise is far below
    assert np.abs(back - p.astype(np.float64)).max() <= 2.0 ** -24 * ext


def test_normalize_flat_and_degenerate():
    p = M.seeded_cloud(257, seed=6)
    p[:, 2] = -0.0
    out, c, s = M.normalize(p)
    assert (out[:, 2] == 0.0).all() and c[2] == 0.0 and not np.signbit(c[2])
    with pytest.raises(ValueError, match='extent 0'):
        M.normalize(np.repeat(p[:1], 5, 0))


def test_prepare_composition():
    p = M.scan_like(1200, seed=9, far=2)
    p[5] = np.nan
    p[77, 1] = np.inf
    out, kept, (c, s), rep = M.prepare(p, max_points=500, thin='voxel', k=8)
    assert rep['points_in'] == 1200 and rep['nonfinite'] == 2 and rep['cropped'] == 2 and rep['outliers'] > 0
    assert rep['points_out'] == kept.size == out.shape[0] <= 500 and rep['R'] >= 1
    assert rep['nonfinite'] + rep['cropped'] + rep['outliers'] + rep['thinned'] + rep['points_out'] == 1200
    assert np.array_equal(out, M.normalize(p[kept])[0])
    out2, kept2, _, rep2 = M.prepare(p, max_points=500, thin='random', k=8, seed=3)
    assert rep2['points_out'] == 500 and np.unique(kept2).size == 500 and rep2['R'] == 0
    # every stage off: the stand-in clouds' arithmetic, the division replaced by a multiplication with 1 / extent
    q = M.seeded_cloud(257, seed=8)
    out3, kept3, _, rep3 = M.prepare(q, crop_quantile=0, std_ratio=0, max_points=0)
    lo, hi = q.astype(np.float64).min(0), q.astype(np.float64).max(0)
    assert np.array_equal(out3, ((q.astype(np.float64) - (lo + hi) * 0.5) * (1.0 / (hi - lo).max())).astype(np.float32))
    assert np.array_equal(kept3, np.arange(257))
