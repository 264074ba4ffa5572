"""tests/components_model.py against independent implementations (scipy's connected_components and cKDTree.query_pairs) on the
cases that tests/test_gpu_components.py runs on the device; ``select`` on hand-written stats; the prepare report's header
with the cluster stage off.  No device."""
import numpy as np
import pytest

import components_model as CM

MESHES = CM.small_cases()
CLOUDS = CM.cluster_cases()


def _scipy_face_labels(v, f):
    """per face the smallest face id of its component, by scipy over the bipartite graph faces -- vertices"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    V, F = len(v), len(f)
    rows = np.repeat(np.arange(F), 3)
    g = coo_matrix((np.ones(3 * F), (rows, F + f.reshape(-1).astype(np.int64))), shape=(F + V, F + V))
    lab = connected_components(g, directed=False)[1][:F]
    first = {}
    for i, c in enumerate(lab.tolist()):
        first.setdefault(c, i)
    return np.array([first[c] for c in lab.tolist()], np.int64)


@pytest.mark.parametrize('name', sorted(MESHES))
def test_mesh_model_against_scipy(name):
    v, f = MESHES[name]
    m = CM.mesh_components(v, f)
    F = len(f)
    assert m['comp'].shape == (F,) and m['report'][0] == len(v) | (F << 32)
    if F == 0:
        assert m['report'][1] == 0 and m['report'][4] == len(v)
        return
    want = _scipy_face_labels(v, f)
    assert np.array_equal(m['counts'][m['comp'], 0], want)
    C = int(m['report'][1])
    assert C == len(set(want.tolist())) and np.all(np.diff(m['counts'][:, 0]) > 0)       # ordered by the smallest face id
    assert m['counts'][:, 1].sum() == F
    assert m['counts'][:, 2].sum() + m['report'][4] == len(v)


def test_the_hand_made_meshes_say_what_the_issue_says():
    c = {k: CM.mesh_components(*MESHES[k]) for k in MESHES}
    assert c['shared_vertex']['report'][1] == 1 and c['same_triangles_separate_indices']['report'][1] == 2
    assert c['quad']['counts'][0].tolist() == [0, 2, 4, 4, 0]
    assert c['three_faces_on_one_edge']['counts'][0].tolist() == [0, 3, 5, 6, 1]
    assert c['unreferenced_at_both_ends']['report'][4] == 6
    r = c['repeated_index']                                  # (1, 1, 2): one edge used once; (3, 4, 3) likewise; (0, 0, 0): none
    assert r['report'][1] == 3 and r['counts'][:, 3].tolist() == [1, 1, 0] and np.all(r['measures'][:, 0] == 0)
    assert r['counts'][:, 2].tolist() == [2, 2, 1]
    t = c['tetra_with_cavity']
    st = CM.stats(t)
    assert st['closed'].tolist() == [True, True] and st['volume'][0] > 0 > st['volume'][1]
    assert abs(st['volume'][0] - 8.0 / 3.0) < 1e-12 and abs(st['volume'][1] + (8.0 / 3.0) / 64.0) < 1e-12
    s = CM.mesh_components(*CM.separate_triangles(70))
    assert np.array_equal(s['comp'], np.arange(70))
    assert CM.mesh_components(*MESHES['strip2000'])['counts'][0].tolist() == [0, 2000, 2002, 2002, 0]


def test_submesh_model():
    v, f = CM.join([CM.tetra(1.0), CM.tetra(0.25, inward=True)])
    vo, fo, src, vmap = CM.submesh(v, f, [0, 0, 0, 0, 1, 0, 1, 1])
    assert src.tolist() == [4, 6, 7] and vmap[:4].tolist() == [-1] * 4 and sorted(set(fo.reshape(-1).tolist())) == [0, 1, 2, 3]
    assert np.array_equal(vo[fo], v[f[src]])
    vo, fo, src, vmap = CM.submesh(v, f, np.zeros(8))
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and np.all(vmap == -1)


@pytest.mark.parametrize('name', sorted(CLOUDS))
def test_cluster_model_against_scipy(name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    p, radius = CLOUDS[name]
    m = CM.clusters(p, radius, 1)
    n = len(p)
    assert m['labels'].shape == (n,) and m['ids'].tolist() == list(range(n)) and m['info'][3] == 0
    if n == 0:
        return
    # the tree's own predicate rounds differently at the radius itself: take its pairs of a slightly larger ball, decide by ours
    pd = p.astype(np.float64)
    cand = cKDTree(pd).query_pairs(radius * (1 + 1e-9), output_type='ndarray').reshape(-1, 2)
    d = pd[cand[:, 0]] - pd[cand[:, 1]]
    near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= radius * radius
    a, b = CM.linked_pairs(p, radius)
    assert sorted(zip(a.tolist(), b.tolist())) == sorted((min(x, y), max(x, y)) for x, y in cand[near].tolist())
    g = coo_matrix((np.ones(int(near.sum())), (cand[near, 0], cand[near, 1])), shape=(n, n))
    k, lab = connected_components(g, directed=False)
    assert k == m['info'][0]
    first = {}
    for i, c in enumerate(lab.tolist()):
        first.setdefault(c, i)
    assert np.array_equal(m['labels'], [first[c] for c in lab.tolist()])


def test_the_hand_made_clouds_say_what_the_issue_says():
    c = {k: CM.clusters(*CLOUDS[k], 1)['info'].tolist() for k in CLOUDS}
    assert c['exactly_radius'][:2] == [1, 2] and c['one_ulp_further'][:2] == [2, 1]
    assert c['star_inside'][:3] == [1, 27, 0]
    assert c['coincident500'][:2] == [1, 500] and c['chain3000'][:2] == [1, 3000]
    assert c['lattice70000'][:2] == [70000, 1] and c['clumps'][:2] == [4, 20000]
    # 26 points on a sphere of the radius cannot be pairwise further apart than the radius: "the partners just outside" is
    # one cloud per partner, two clusters each; in the cloud of all of them the centre is alone
    p, r = CLOUDS['star_outside']
    for k in range(1, 27):
        assert CM.clusters(p[[0, k]], r, 1)['info'][:2].tolist() == [2, 1]
    lab = CM.clusters(p, r, 1)['labels']
    assert (lab == 0).sum() == 1


@pytest.mark.parametrize('min_points,gone', [(1, 0), (6, 1), (51, 2), (301, 3), (10 ** 6, 3)])
def test_cluster_keep_rule(min_points, gone):
    p, r = CLOUDS['clumps']
    m = CM.clusters(p, r, min_points)
    assert m['info'].tolist()[:2] == [4, 20000] and m['info'][3] == gone
    assert len(m['ids']) == 20355 - sum((5, 50, 300)[:gone])


def _stats(faces, area, first=None):
    C = len(faces)
    z = np.zeros(C, np.int64)
    return dict(first_face=np.arange(C) * 10 if first is None else np.asarray(first), faces=np.asarray(faces), vertices=z, boundary_edges=z,
                nonmanifold_edges=z, area=np.asarray(area, np.float64), volume=np.zeros(C), box_lo=np.zeros((C, 3)), box_hi=np.zeros((C, 3)),
                closed=np.ones(C, bool))


def test_select():
    from points2surf_amd import components
    for sel in (components.select, CM.select):
        st = _stats([100, 5, 50, 7], [10.0, 0.05, 3.0, 0.1])
        assert sel(st).tolist() == [True] * 4
        assert sel(st, min_faces=6).tolist() == [True, False, True, True]
        assert sel(st, min_area_share=0.01).tolist() == [True, False, True, True]       # 0.1 >= 0.01 * 10 holds, 0.05 does not
        assert sel(st, min_area_share=0.01, max_components=2).tolist() == [True, False, True, False]
        assert sel(st, max_components=1).tolist() == [True, False, False, False]
        # the largest area survives a min_faces it fails
        assert sel(_stats([3, 500], [9.0, 1.0]), min_faces=10).tolist() == [True, True]
        assert sel(_stats([3, 5], [9.0, 1.0]), min_faces=10).tolist() == [True, False]
        # equal areas: the smaller first face wins, whatever the rank
        tie = _stats([4, 4, 4], [2.0, 2.0, 2.0], first=[30, 10, 20])
        assert sel(tie, max_components=1).tolist() == [False, True, False]
        assert sel(tie, max_components=2).tolist() == [False, True, True]
        assert sel(tie, min_faces=99).tolist() == [False, True, False]
        assert sel(_stats([], [])).shape == (0,)
    with pytest.raises(ValueError):
        components.select(_stats([1], [1.0]), min_area_share=1.5)
    with pytest.raises(ValueError):
        components.select(_stats([1], [1.0]), min_faces=-1)


def test_select_agrees_with_the_model_on_random_stats():
    from points2surf_amd import components
    rng = np.random.RandomState(0)
    for _ in range(200):
        C = int(rng.randint(1, 9))
        st = _stats(rng.randint(1, 20, C), rng.randint(0, 4, C).astype(np.float64), first=rng.permutation(C))
        kw = dict(min_faces=int(rng.randint(0, 20)), min_area_share=float(rng.choice([0.0, 0.3, 1.0])), max_components=int(rng.randint(0, 4)))
        assert components.select(st, **kw).tolist() == CM.select(st, **kw).tolist(), (st, kw)


def test_prepare_report_header_is_unchanged_with_the_stage_off():
    from points2surf_amd import prepare
    assert prepare.REPORT_COLUMNS == ('file', 'points_in', 'nonfinite', 'cropped', 'outliers', 'thinned', 'points_out', 'R', 'mean', 'std',
                                      'threshold', 'centre_x', 'centre_y', 'centre_z', 'scale', 'refused')
    assert (prepare.DEFAULTS['min_cluster'], prepare.DEFAULTS['cluster_radius'], prepare.DEFAULTS['cluster_factor']) == (0, 0.0, 3.0)
    assert list(prepare._row('a.ply', dict(points_in=3, clusters=2, small_clusters=1))) == list(prepare.REPORT_COLUMNS)
    with pytest.raises(ValueError, match='--cluster_radius'):
        prepare.prepare(np.zeros((4, 3), np.float32), std_ratio=0.0, min_cluster=5)
