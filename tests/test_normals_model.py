"""The float64 model of the normal estimation and orientation (tests/normals_model.py) on clouds with analytic normals:
Hoppe's rule, as the device applies it, must orient EVERY point outward there.  This keeps the condition of the GPU tests
(tests/test_gpu_normals.py) true for the seeds fixed in the model, and checks the model's own parts against plain
restatements."""
import numpy as np
import pytest

import normals_model as M

CLOUDS = {'sphere': M.sphere, 'torus': M.torus, 'noisy_sphere': M.noisy_sphere}


@pytest.mark.parametrize('k', [8, 12, 16])
@pytest.mark.parametrize('name', sorted(CLOUDS))
def test_model_orients_every_point_outward(name, k):
    pts, truth = CLOUDS[name]()
    nrm, comp, info, _ = M.oriented(pts, k)
    dot = (nrm.astype(np.float64) * truth).sum(axis=1)
    print(name, 'k', k, 'components', info['components'], 'wrong', int((dot <= 0).sum()), 'worst |dot|', float(np.abs(dot).min()))
    assert info['components'] == 1 and (comp == 0).all()
    assert (dot > 0).all()


def test_model_two_spheres_two_components():
    pts, truth = M.two_spheres()
    nrm, comp, info, _ = M.oriented(pts, 12)
    dot = (nrm.astype(np.float64) * truth).sum(axis=1)
    assert info['components'] == 2
    assert set(np.unique(comp)) == {0, 2000} and (comp[:2000] == 0).all() and (comp[2000:] == 2000).all()
    for part in (slice(0, 2000), slice(2000, None)):
        assert int((dot[part] <= 0).sum()) == 0


def test_knn_ties_go_to_the_smaller_id():
    rng = np.random.default_rng(1)
    base = rng.uniform(-0.5, 0.5, (60, 3)).astype(np.float32)
    pts = np.concatenate([base, base])                   # every point twice: id i and id i + 60 at distance 0 of each other
    ids = M.knn(pts, 4)
    assert (ids[:60, 0] == np.arange(60)).all() and (ids[:60, 1] == np.arange(60) + 60).all()
    assert (ids[60:, 0] == np.arange(60)).all() and (ids[60:, 1] == np.arange(60) + 60).all()
    p = pts.astype(np.float64)
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1)
    for i in (0, 17, 119):
        want = sorted(range(120), key=lambda j: (d2[i, j], j))[:4]
        assert list(ids[i]) == want


def test_tree_knn_equals_the_brute_force():
    pts = M.noisy_sphere()[0]
    pts[100:103] = pts[7]                                # ties at distance 0
    assert np.array_equal(M.knn_tree(pts, 12), M.knn(pts, 12))


def test_orient_is_kruskal_in_the_total_order():
    """a 3 x 3 grid in the plane z = 0 with normals +-(0, 0, 1): every weight ties at 0, the ids alone decide the forest, and
    whatever forest it is the result is all +z; a zero normal never flips its neighbours (d = 0)"""
    g = np.stack(np.meshgrid(np.arange(3.0), np.arange(3.0), indexing='ij'), -1).reshape(-1, 2)
    pts = np.concatenate([g, np.zeros((9, 1))], axis=1).astype(np.float32)
    nrm = np.zeros((9, 3), np.float32)
    nrm[:, 2] = [1, -1, 1, -1, -1, 1, 1, 1, -1]
    out, comp, info = M.orient(pts, nrm, k=4)
    assert (out[:, 2] == 1).all() and (out[:, :2] == 0).all() and (comp == 0).all()
    assert info == dict(components=1, edges=info['edges'], flipped=4)
    nrm[4] = 0.0
    out, _, _ = M.orient(pts, nrm, k=4)
    assert (np.abs(out) == np.abs(nrm)).all()


def test_estimate_on_a_plane_and_on_coincident_points():
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(-0.5, 0.5, (200, 2)), np.zeros((200, 1))], axis=1).astype(np.float32)
    nrm, var, C, lam, _ = M.estimate(pts, 8)
    assert (np.abs(nrm[:, 2]) > 1.0 - 1e-15).all() and (var < 1e-15).all()
    pts[:8] = pts[0]
    nrm, var, _, _, _ = M.estimate(pts, 8)
    assert (nrm[:8] == 0.0).all() and (var[:8] == 0.0).all() and (np.abs(nrm[8:, 2]) > 1.0 - 1e-15).all()
