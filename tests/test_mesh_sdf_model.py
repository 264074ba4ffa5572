"""The float64 CPU model of the mesh-distance kernels (tests/mesh_sdf_model.py) against the reference's recorded GT data
(tests/golden/abc_minimal: 03_meshes, 05_query_pts, 05_query_dist -- byte copies of the reference's data set) and on
constructed cases.  No device, no reference checkout."""
import glob
import os

import numpy as np
import pytest

import mesh_sdf_model as msm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'abc_minimal')
MESHES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, '03_meshes', '*.ply')))


def load(name):
    from points2surf_amd import ply
    v, f = ply.read_ply(os.path.join(GOLDEN, '03_meshes', name))
    q = np.load(os.path.join(GOLDEN, '05_query_pts', name + '.npy'))
    g = np.load(os.path.join(GOLDEN, '05_query_dist', name + '.npy'))
    return np.asarray(v, np.float32), np.asarray(f, np.int64), q, g


@pytest.fixture(scope='module')
def fixture_results():
    out = {}
    for name in MESHES:
        v, f, q, g = load(name)
        m = msm.MeshModel(v, f)
        d, det = m.signed_distance(q.astype(np.float64), with_details=True)
        out[name] = (m, q, g, d, det)
    return out


def test_three_fixture_meshes():
    assert len(MESHES) == 3


def test_fixture_meshes_are_closed_and_consistently_oriented():
    """every edge of the three meshes has exactly two faces, traversing it in opposite directions"""
    for name in MESHES:
        v, f, _, _ = load(name)
        _, fwd, bwd = msm.edge_census(f, len(v))
        assert (fwd == 1).all() and (bwd == 1).all(), name
        m = msm.MeshModel(v, f)
        assert m.closed and m.bad_edges == 0 and (m.adj >= 0).all()
        # neighbours are mutual
        for e in range(3):
            assert (m.adj[m.adj[:, e]] == np.arange(len(f))[:, None]).any(1).all()


def test_model_distance_against_the_recorded_distances(fixture_results):
    """the ceilings measured for exact float64 arithmetic against the reference's recorded |d| (float32 of trimesh's
    result on the float64 query points): max 8.04e-6, three queries beyond 1e-6, 28 beyond 2e-7"""
    err = np.concatenate([np.abs(np.abs(d) - np.abs(g.astype(np.float64))) for _, _, g, d, _ in fixture_results.values()])
    assert len(err) == 6000
    print('max', err.max(), '>1e-6', int((err > 1e-6).sum()), '>2e-7', int((err > 2e-7).sum()))
    assert err.max() <= 1e-5
    assert (err > 1e-6).sum() <= 3
    assert (err > 2e-7).sum() <= 28


def test_winding_sign_equals_the_recorded_sign(fixture_results):
    for name, (m, q, g, _, _) in fixture_results.items():
        w = msm.winding(q.astype(np.float64), m.tri)
        assert np.abs(w - np.round(w)).max() < 1e-9, name
        assert ((np.abs(w) > 0.5) == (g > 0)).all(), name


def test_pseudonormal_sign_equals_the_winding_sign(fixture_results):
    """the pseudonormal sign equals the winding sign on all 6,000 fixture queries.  00011084 is a union of two OVERLAPPING
    closed components: the pseudonormal of the globally nearest feature is the wrong sign for 170 of its 2,000 queries
    (just outside one component, inside the other), which is why the sign of a multi-component mesh is the sum of the
    per-component pseudonormal signs (MeshModel.pseudonormal_sign, p2s_md_comp_sign_kernel)"""
    bad = {}
    for name, (m, q, g, d, det) in fixture_results.items():
        q64 = q.astype(np.float64)
        inside, untrusted = m.pseudonormal_sign(q64)
        w = msm.winding(q64, m.tri)
        bad[name[:8]] = (int((inside != (np.abs(w) > 0.5)).sum()), int(untrusted.sum()))
    print('pseudonormal != winding, untrusted, per mesh:', bad)
    assert all(b == (0, 0) for b in bad.values()), bad


def test_nearest_feature_alone_misses_on_overlapping_components(fixture_results):
    m, q, g, d, det = fixture_results[MESHES[0]]
    outside, _ = m.sign(q.astype(np.float64), det['face'], det['closest'], det['feat'], np.sqrt(det['d2']))
    assert MESHES[0].startswith('00011084') and int((outside != ~(g > 0)).sum()) == 170


def test_entry_point_sign_equals_the_recorded_sign(fixture_results):
    for name, (m, q, g, d, det) in fixture_results.items():
        assert ((d > 0) == (g > 0)).all(), name
        assert set(np.unique(det['feat'])) <= set(range(7))
        assert not det['flagged'].any(), name


def test_overlapping_components_of_00011084(fixture_results):
    comps = {name[:8]: m.components for name, (m, *_r) in fixture_results.items()}
    print('components', comps)
    assert comps == {'00011084': 2, '00016513': 1, '00994122': 2}


def test_constructed_queries_on_an_l_shaped_prism():
    """on the normal line of a vertex, over an edge midpoint at a reflex and at a convex edge, 1e-7 from a face"""
    v, f = msm.l_prism()
    m = msm.MeshModel(v, f)
    assert m.closed and not m.inverted
    t = 0.25
    s3 = 1 / np.sqrt(3)
    q = np.array([
        [-t * s3, -t * s3, -t * s3],          # 0 outside, on the normal line of the convex vertex (0, 0, 0)
        [2 + t * s3, -t * s3, 1 + t * s3],    # 1 outside, vertex (2, 0, 1)
        [1 + 0.1, 1 + 0.1, 0.5],              # 2 outside, in the notch beside the reflex edge x = y = 1: a face is nearer
        [1 - 0.1, 1 - 0.1, 0.5],              # 3 inside, closest to the reflex edge
        [2 + 0.1, -0.1, 0.5],                 # 4 outside, over the midpoint of the convex edge (2, 0, z)
        [0.5, 0.3, 1 + 1e-7],                 # 5 outside, 1e-7 above the top face
        [0.5, 0.3, 1 - 1e-7],                 # 6 inside, 1e-7 below it
        [0.5, 0.3, 1 + 1e-9],                 # 7 within tol.merge: unsigned
    ])
    d, det = m.signed_distance(q, with_details=True)
    feat = det['feat']
    assert feat[0] >= 4 and feat[1] >= 4 and feat[2] == 0 and 1 <= feat[3] <= 3 and 1 <= feat[4] <= 3
    assert feat[5] == 0 and feat[6] == 0
    assert not det['flagged'].any()
    want = np.array([-t, -t, -0.1, 0.1 * np.sqrt(2), -0.1 * np.sqrt(2), -1e-7, 1e-7, 1e-9])
    assert np.abs(d - want).max() < 1e-12
    w = msm.winding(q[:7], m.tri)
    assert ((np.abs(w) > 0.5) == (d[:7] > 0)).all()
    # the same mesh turned inside out is recognised and gives the same signed distances
    mi = msm.MeshModel(v, f[:, [0, 2, 1]])
    assert mi.closed and mi.inverted
    assert np.array_equal(mi.signed_distance(q), d)
    # one face removed: three open edges
    mo = msm.MeshModel(v, f[1:])
    assert not mo.closed and mo.bad_edges == 3


def test_tie_goes_to_the_smallest_face_id_and_degenerate_faces_are_segments():
    v, f = msm.l_prism()
    d2, face, _, feat, second = msm.nearest(v, f, np.array([[-1.0, -1.0, -1.0]]))
    touching = np.nonzero((f == 0).any(1))[0]
    assert face[0] == touching.min() and feat[0] >= 4 and second[0] == d2[0]
    # zero-area triangles (two coincident corners, three collinear corners): finite, the distance of the segment
    T = np.array([[0, 0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 2, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0]], np.float64)
    P = np.array([[0.5, 1.0, 0.0], [1.5, 0.0, 2.0], [0.0, 3.0, 4.0]])
    d2, c, feat = msm.tri_closest(P, T)
    assert np.isfinite(d2).all() and np.isfinite(c).all()
    assert np.allclose(d2, [1.0, 4.0, 25.0], atol=0, rtol=1e-15) and (feat > 0).all()


def test_regions_agree_with_plane_projection():
    """a second formulation: where the closest feature is the face, the distance is the distance to the plane"""
    rng = np.random.RandomState(5)
    T = rng.uniform(-1, 1, (20000, 9))
    P = rng.uniform(-1, 1, (20000, 3))
    d2, c, feat = msm.tri_closest(P, T)
    A = T[:, :3]
    n = msm.cross3(T[:, 3:6] - A, T[:, 6:9] - A)
    plane = msm.dot3(n, P - A) ** 2 / msm.dot3(n, n)
    on_face = (feat == 0) & (msm.dot3(n, n) > 1e-4)
    assert on_face.sum() > 1000
    print('regions vs plane projection: max |d2 difference|', np.abs(d2 - plane)[on_face].max())
    assert np.abs(d2 - plane)[on_face].max() < 2.5e-14          # -> the 1e-13 bound of the device test stands
    # and no point of the triangle is nearer than the reported one (sampled)
    bary = rng.dirichlet((1, 1, 1), 20000)
    s = bary[:, :1] * T[:, :3] + bary[:, 1:2] * T[:, 3:6] + bary[:, 2:] * T[:, 6:9]
    assert (((P - s) ** 2).sum(1) >= d2 - 1e-12).all()


def test_query_dist_post_processing():
    d = np.array([np.nan, np.inf, -np.inf, -3.0, 2.0, 0.25, -0.5, 1e-9, -1.0000001])
    want = d.copy()
    want[np.isnan(d)] = 0.0
    want[np.isinf(d)] = 1.0
    want = np.clip(want, -1.0, 1.0).astype(np.float32)
    got = msm.query_dist_post(d)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.isnan(d[0])                       # the input is not modified
