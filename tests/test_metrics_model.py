"""CPU: tests/metrics_model.py against oracle/metrics_oracle.py (scipy's query_pairs, cKDTree.query and
directed_hausdorff, the trimesh restatement), and every recipe against what its docstring claims -- so that
tests/test_gpu_metrics_edges.py compares the device with a model that is pinned, on inputs that are known to reach the
mechanism they aim at.  Conditions on the inputs of the GPU tests (the 0.1 % leave-out rule, no pair at the rejection
radius of the even sampling) are checked here, by the oracle alone."""
import math
import os

import numpy as np
import pytest
import scipy.spatial as spatial

import metrics_model as M
from oracle import metrics_oracle as MO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = os.path.join(REPO, 'tests', 'golden', 'abc_minimal', '03_meshes')
NAMES = ['00011084_fddd53ce45f640f3ab922328_trimesh_019', '00016513_3d6966cd42eb44ab8f4224f2_trimesh_053',
         '00994122_57d9d4755722f9d2d7436f0a_trimesh_000']


def _fixture_mesh(i):
    from points2surf_amd import ply
    v, f = ply.read_ply(os.path.join(MESHES, NAMES[i] + '.ply'))
    return v.astype(np.float32), f.astype(np.int32)


# ---- remove_close ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', M.REMOVE_CLOSE_INPUTS)
def test_remove_close_model_is_the_oracle_on_every_recipe_and_size(name):
    """masks equal scipy's query_pairs + the trimesh rule at every m the GPU test runs, exact-radius pairs and r = 0
    included"""
    for m in M.M_LIST:
        pts, radius = M.remove_close_input(name, m)
        assert pts.shape == (m, 3) and pts.dtype == np.float32
        keep, degree = M.remove_close_model(pts, radius)
        kept_ref, mask_ref = MO.remove_close(pts, radius)
        assert np.array_equal(keep, mask_ref), (name, m)
        assert np.array_equal(pts[keep], kept_ref)
        pairs = spatial.cKDTree(pts.astype(np.float64)).query_pairs(radius, output_type='ndarray')
        assert np.array_equal(degree, np.bincount(pairs.ravel(), minlength=m)), (name, m)


def test_lattice_points_pairs_exactly_at_the_radius_and_degree_ties():
    h = 2.0 ** -5
    pts = M.lattice_points(9, h)
    assert pts.shape == (729, 3)
    at_h = M.close_pairs(pts, h)
    assert len(at_h) == 1944 == 3 * 9 * 9 * 8                                      # the axis neighbours, all exactly at h
    p = pts.astype(np.float64)
    d2 = ((p[at_h[:, 0]] - p[at_h[:, 1]]) ** 2).sum(axis=1)
    assert np.all(d2 == h * h)                                                      # `<` instead of `<=` loses every one
    assert len(M.close_pairs(pts, h * (1.0 - 2.0 ** -30))) == 0
    assert len(spatial.cKDTree(p).query_pairs(h)) == 1944
    at_2h = M.close_pairs(pts, 2.0 * h)
    d2 = ((p[at_2h[:, 0]] - p[at_2h[:, 1]]) ** 2).sum(axis=1)
    assert set(np.unique(d2 / (h * h)).tolist()) == {1.0, 2.0, 3.0, 4.0}
    assert np.count_nonzero(d2 == 4.0 * h * h) == 3 * 9 * 9 * 7                     # exactly at 2h
    for r in (h, 2.0 * h):
        pr = M.close_pairs(pts, r)
        deg = M.remove_close_model(pts, r)[1]
        ties = np.count_nonzero(deg[pr[:, 0]] == deg[pr[:, 1]])
        assert ties > len(pr) // 4 and ties < len(pr)                               # both arms of the tie rule
        assert deg.max() == (6 if r == h else 32)
    # the cut to m points of the GPU test keeps both properties
    for m in (255, 257, 1025, 3000):
        pts, r = M.remove_close_input('lattice_h', m)
        pr = M.close_pairs(pts, r)
        deg = M.remove_close_model(pts, r)[1]
        assert len(pr) > m // 2 and np.count_nonzero(deg[pr[:, 0]] == deg[pr[:, 1]]) > 0
        assert np.count_nonzero(deg[pr[:, 0]] > deg[pr[:, 1]]) > 0 and np.count_nonzero(deg[pr[:, 0]] < deg[pr[:, 1]]) > 0


def test_clustered_points_degrees_above_a_tile_and_duplicate_stacks():
    for m in (1024, 1400, 3000):
        pts, is_stack = M.clustered_points(m)
        keep, deg = M.remove_close_model(pts, 0.02)
        assert deg.max() > 256, (m, deg.max())                                      # more partners than one LDS tile holds
        assert 0 < keep.sum() < m
        # radius 0: the close pairs are the pairs of exact duplicates; of each stack of five the last one stays
        keep0, deg0 = M.remove_close_model(pts, 0.0)
        assert np.array_equal(deg0 > 0, is_stack) and set(deg0[is_stack].tolist()) == {4}
        assert keep0.sum() == m - is_stack.sum() + is_stack.sum() // 5
        _, first = np.unique(pts[::-1], axis=0, return_index=True)
        assert np.array_equal(np.sort(m - 1 - first), np.nonzero(keep0)[0])
    # the cluster is spread over the tiles: close pairs between the first and the last tile
    pts, _ = M.clustered_points(3000)
    pr = M.close_pairs(pts, 0.02)
    assert np.any((pr[:, 0] < 256) & (pr[:, 1] >= 2816))


def test_straddling_points_pairs_are_the_only_close_pairs():
    for m in M.M_LIST:
        pts, pairs, r = M.straddling_points(m)
        assert np.array_equal(M.close_pairs(pts, r), pairs), m
        have = set(map(tuple, pairs.tolist()))
        if m >= 2:
            assert (0, m - 1) in have
        if m > 256:
            assert (255, 256) in have
        for t in range(1, (m - 1) // 256 + 1):
            assert (256 * t - 1, 256 * t) in have or m - 1 == 256 * t and (0, m - 1) in have
        if m % 256 >= 4:
            assert any(a // 256 == b // 256 == (m - 1) // 256 for a, b in have)      # inside the partial last tile
        p = pts.astype(np.float64)
        far = spatial.cKDTree(p).query_pairs(0.9, output_type='ndarray')
        assert len(far) == len(pairs)                                               # everything else is a unit apart


# ---- nearest-neighbour statistics --------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(M.nn_targets()))
def test_nn_model_is_scipy(name):
    """bit for bit: the model, cKDTree.query and directed_hausdorff all take sqrt of the same sum (dx*dx + dy*dy) + dz*dz
    of the same float64 differences, and the minimum over the targets does not depend on the order they are visited"""
    t = M.nn_targets()[name]
    for n in (1, 65, 1025):
        q = M.nn_queries(t, n)
        dist, mx, sm = M.nn_model(q, t)
        q64, t64 = q.astype(np.float64), t.astype(np.float64)
        assert np.array_equal(dist, spatial.cKDTree(t64).query(q64, 1)[0]), (name, n)
        assert mx == spatial.distance.directed_hausdorff(q64, t64)[0]
        assert sm == math.fsum(dist.tolist()) and abs(sm - float(np.sum(dist))) <= (n - 1) * 2.0 ** -53 * sm
        assert np.all(dist[1::4] == 0.0)                                             # the target's own points
        if n >= 65:
            lo, hi = t64.min(axis=0), t64.max(axis=0)
            outside = np.any((q64 < lo) | (q64 > hi), axis=1)
            assert outside[0::4].all() and dist[0::4].min() > 0.0 and dist[64] > 0.0
            assert np.any(np.signbit(q) & (q == 0.0))                                # -0.0 coordinates are there


def test_nn_queries_far_query_is_the_single_largest_distance():
    t = M.nn_targets()['coplanar']
    for at in (0, 1023, 1024, 2048):
        dist = M.nn_model(M.nn_queries(t, 2049, far_at=at), t)[0]
        assert int(np.argmax(dist)) == at and np.count_nonzero(dist == dist.max()) == 1


def test_outlier_sets_known_answers():
    for name, a, b, (h_ab, s_ab, h_ba, s_ba) in M.outlier_sets():
        d_ab, mx_ab, sm_ab = M.nn_model(a, b)
        d_ba, mx_ba, sm_ba = M.nn_model(b, a)
        assert (mx_ab, sm_ab, mx_ba, sm_ba) == (h_ab, s_ab, h_ba, s_ba), name
        assert float(np.sum(d_ab)) == s_ab and float(np.sum(d_ba[::-1])) == s_ba     # exact in any order
        ref = MO.mesh_distances(a, b)
        assert ref == (h_ab, h_ba, max(h_ab, h_ba), s_ab + s_ba)
        assert np.argmax(d_ba) == len(b) - 1                                         # the outlier decides


# ---- sampling ----------------------------------------------------------------------------------------------------------

EXACT_NF = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)


@pytest.mark.parametrize('nf', EXACT_NF)
def test_lattice_mesh_areas_and_all_partial_sums_are_exact(nf):
    for deg in ({}, M.degenerate_positions(nf)):
        v, f = M.lattice_mesh(nf, deg)
        area = M.face_areas(v, f)
        units = area * 2.0 ** 17
        assert np.array_equal(units, np.round(units)) and units.max() <= 25
        assert np.array_equal(area == 0.0, np.array([k in deg for k in range(nf)]))
        assert len(set(units[units > 0].tolist())) >= min(nf - len(deg), 6)          # several different areas
        cum = np.cumsum(area)
        prefix = np.array([math.fsum(area[:k + 1].tolist()) for k in range(0, nf, max(1, nf // 97))] + [math.fsum(area.tolist())])
        assert np.array_equal(cum[list(range(0, nf, max(1, nf // 97))) + [nf - 1]], prefix)
        assert float(np.sum(area[::-1])) == cum[-1] == float(np.sum(np.sort(area)))   # any order
    deg = M.degenerate_positions(nf)
    if nf > 2:
        assert 0 in deg and nf - 1 in deg and set(deg.values()) == {'repeat', 'collinear'}
    if nf > 1025:
        assert 1023 in deg and 1024 in deg
    if nf >= 63:
        assert all(k in deg for k in range(nf // 3, nf // 3 + 5))                    # a run
    v, f = M.lattice_mesh(nf, deg)
    assert all((f[k, 1] == f[k, 2]) == (kind == 'repeat') for k, kind in deg.items())


@pytest.mark.parametrize('which', ['lattice', 'lattice degenerate', 'fixture'])
def test_sample_model_is_the_oracle(which):
    if which == 'fixture':
        v, f = _fixture_mesh(2)
    else:
        v, f = M.lattice_mesh(1025, M.degenerate_positions(1025) if 'degenerate' in which else None)
    rs, twin = np.random.RandomState(7), np.random.RandomState(7)
    for count in (1, 257, 3000):
        ref, area_ref, idx_ref = MO.sample_surface(v, f, count, rs)
        pts, face, area, cum = M.sample_model(v, f, twin.random_sample(3 * count))
        assert np.array_equal(face, idx_ref) and area == area_ref
        assert np.array_equal(pts, ref)                                              # (e1 l1 + e2 l2) + o, rounded once
        assert np.array_equal(M.searchsorted_left(cum, twin.random_sample(50) * cum[-1]), np.searchsorted(cum, rs.random_sample(50) * cum[-1]))
        if 'degenerate' in which:
            assert np.all(M.face_areas(v, f)[face] > 0.0)


def test_fed_deviates_reach_the_edges():
    nf = 1025
    deg = M.degenerate_positions(nf)
    v, f = M.lattice_mesh(nf, deg)
    cum = np.cumsum(M.face_areas(v, f))
    u, exact_k, n = M.fed_deviates(cum)
    pts, face, area, _ = M.sample_model(v, f, u)
    picks, l1, l2 = u[:n], u[n::2], u[n + 1::2]
    assert np.all(face[picks == 0.0] == 0) and 0 in deg                              # pick 0.0: the first face, a degenerate one
    last_with_area = max(k for k in range(nf) if k not in deg)
    assert np.all(face[picks == 1.0 - 2.0 ** -53] == last_with_area) and nf - 1 in deg
    # picks exactly on a cumulative value take the face that ENDS there (left), also where zero-area faces repeat it
    assert len(exact_k) > nf // 2
    hit = dict((float(cum[k]), k) for k in reversed(exact_k))                        # the first k of a repeated value
    on = np.isin(picks * cum[-1], cum) & (np.arange(n) >= 30)                        # after the three special picks
    assert on.sum() == len(exact_k) * 10
    assert all(face[s] == hit[float(picks[s] * cum[-1])] for s in np.nonzero(on)[0])
    right = np.searchsorted(cum, picks[on] * cum[-1], 'right')
    assert np.all(right > face[on])                                                  # searchsorted-right differs on every one
    before_run = [k for k in exact_k if k + 1 in deg and k not in deg]
    assert len(before_run) == 2 and all(k + 2 in deg for k in before_run)           # in front of the two runs
    # folds: sums of exactly 1.0 stay, 1 + 2^-53 rounds to 1.0 and stays, one ulp above 1 folds
    s = l1 + l2
    assert np.count_nonzero(s == 1.0) >= 4 * (n // 10) and np.count_nonzero(s == 1.0 + 2.0 ** -52) == 2 * (n // 10)
    assert np.any((l2 == 0.75 + 2.0 ** -53) & (s == 1.0))
    # one ulp in a length decides the fold, and the fold moves the point across the triangle (a wrong decision shows)
    first = 2 * 10                                                                   # the samples of pick 0.5, one per pair
    assert len(set(face[first:first + 10].tolist())) == 1 and M.face_areas(v, f)[face[first]] > 0.0
    assert np.array_equal(pts[first], pts[first + 3]) and not np.array_equal(pts[first + 3], pts[first + 4])
    assert np.abs(pts[first + 3] - pts[first + 4]).max() >= 2.0 ** -10


@pytest.mark.parametrize('i', [0, 1, 2])
def test_leave_out_condition_of_the_fixture_meshes(i):
    """the GPU test compares face ids only where the pick lies further than nf * 2^-53 * total from every cumulative
    value; with seed M.FIXTURE_SEED and 5000 samples that leaves out less than 0.1 % -- by the oracle's numbers alone"""
    v, f = _fixture_mesh(i)
    nf, count = len(f), 5000
    rs = np.random.RandomState(M.FIXTURE_SEED)
    _, area_ref, idx_ref = MO.sample_surface(v, f, count, rs)
    tri = v.astype(np.float64)[f]
    cum = np.cumsum(np.sqrt((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(axis=1)) / 2.0)
    assert cum[-1] == area_ref
    picks = np.random.RandomState(M.FIXTURE_SEED).random_sample(count)
    assert np.array_equal(np.minimum(np.searchsorted(cum, picks * cum[-1]), nf - 1), idx_ref)
    left_out = M.boundary_margin(cum, picks) <= nf * 2.0 ** -53 * cum[-1]
    assert left_out.mean() < 0.001
    assert np.array_equal(cum, M.sample_model(v, f, np.zeros(3))[3])                 # the model's areas are the oracle's
    assert abs(cum[-1] - math.fsum(M.face_areas(v, f).tolist())) <= nf * 2.0 ** -53 * cum[-1]


@pytest.mark.parametrize('which', ['lattice', 'fixture'])
def test_even_sampling_inputs_are_decided(which):
    """the end-to-end GPU test asserts row equality with the oracle; that needs (1) every one of the 3 * count face picks
    away from the cumulative boundaries (fixture mesh; the lattice mesh is exact), and (2) no candidate pair so close to
    the rejection radius that the last bits of the area could decide it"""
    count = 300
    v, f = M.even_lattice_mesh() if which == 'lattice' else _fixture_mesh(2)
    rs = np.random.RandomState(M.EVEN_SEED)
    cand, area, _ = MO.sample_surface(v, f, 3 * count, rs)
    cum = np.cumsum(M.face_areas(v, f))
    picks = np.random.RandomState(M.EVEN_SEED).random_sample(3 * count)
    assert np.all(M.boundary_margin(cum, picks) > len(f) * 2.0 ** -53 * cum[-1])
    r2 = area / (3 * count)
    p = cand.astype(np.float64)
    d2 = np.concatenate([M._d2_block(p[i0:i0 + 256], p).ravel() for i0 in range(0, len(p), 256)])
    # the device's area and the oracle's each lie within nf * 2^-53 relative of the exact one, and r2 with them
    assert not np.any(np.abs(d2 - r2) <= 2 * len(f) * 2.0 ** -53 * r2)
    out = MO.sample_surface_even(v, f, count, np.random.RandomState(M.EVEN_SEED))
    assert 0 < len(out) <= count
    keep, _ = M.remove_close_model(cand, np.sqrt(r2))
    assert np.array_equal(cand[keep][:count], out)
    assert keep.sum() > count                                   # the cut to count (compact_points_kernel's limit) is taken
