"""The CPU model of p2s_mesh_check (tests/mesh_check_model.py) against constructions with known answers, and the premise
of the check: on a mesh that passes through itself inside ONE component the pseudonormal sign is wrong where the winding
number is right."""
import numpy as np
import pytest

import clean_model
import mesh_check_model as M
import mesh_sdf_model

# name -> (mesh, intersecting, coplanar, touching, non-manifold vertices)
CASES = {
    'crossing': (M.crossing, 1, 0, 0, 0),
    'apart': (M.apart, 0, 0, 0, 0),
    'shared_vertex_pierce': (M.shared_vertex_pierce, 1, 0, 0, 1),      # two faces on one vertex are no fan
    'adjacent': (M.adjacent, 0, 0, 0, 0),
    'fold': (M.fold, 0, 1, 0, 0),
    'coplanar_overlap': (M.coplanar_overlap, 0, 1, 0, 0),
    'coplanar_apart': (M.coplanar_apart, 0, 0, 0, 0),
    'vertex_on_face': (M.vertex_on_face, 0, 0, 1, 0),
    'bowtie': (M.bowtie, 0, 0, 0, 1),
    'cube': (clean_model.cube, 0, 0, 0, 0),
    'icosahedron': (clean_model.icosahedron, 0, 0, 0, 0),
    'moebius': (clean_model.moebius, 0, 0, 0, 0),
}

@pytest.mark.parametrize('name', sorted(CASES))
def test_known_answers(name):
    make, n_int, n_cop, n_touch, n_nm = CASES[name]
    v, f = make()
    r = M.check(v, f)
    rep = r['report']
    assert (rep['intersecting'], rep['coplanar'], rep['touching'], rep['nonmanifold_vertices']) == (n_int, n_cop, n_touch, n_nm), rep
    assert rep['duplicate'] == 0 and rep['faces_degenerate'] == 0 and rep['pairs_stored'] == n_int + n_cop + n_touch
    assert len(r['pairs']) == rep['pairs_stored'] and (r['pairs'][:, 0] < r['pairs'][:, 1]).all()
    assert rep['faces_flagged'] == 2 * (n_int + n_cop)
    if name == 'bowtie':
        assert r['vert_flags'].tolist() == [1, 0, 0, 0, 0, 0, 0]


def test_duplicates_and_degenerate_faces_are_counted_not_tested():
    v = np.array(M.T0 + [[1, 1, 0]], np.float32)
    f = np.array([[0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 3, 3], [0, 1, 3]], np.int32)     # three copies, one collapsed face, one more
    r = M.check(v, f)['report']
    assert r['faces_degenerate'] == 1 and r['faces_tested'] == 4 and r['duplicate'] == 3


def test_pairs_are_ordered_and_symmetric_in_the_faces():
    """the class of a pair does not depend on which face comes first, except through the axis that is dropped"""
    v, f = M.ribbon_prism()
    a = M.check(v, f)
    p = a['pairs'].astype(np.int64)
    assert (np.diff(p[:, 0] * len(f) + p[:, 1]) > 0).all()
    perm = np.arange(len(f))[::-1]
    b = M.check(v, f[perm])
    back = np.sort(perm[b['pairs'].astype(np.int64)], axis=1)
    order = np.lexsort((back[:, 1], back[:, 0]))
    assert np.array_equal(back[order], p) and np.array_equal(b['classes'][order], a['classes'])


def test_ribbon_prism_is_a_volume_that_passes_through_itself():
    v, f = M.ribbon_prism()
    out_v, out_f, _, rep = clean_model.repair(v, f)
    assert rep['is_volume'] == 1 and rep['components'] == 1 and len(out_f) == len(f)
    r = M.check(v, f)['report']
    assert r['intersecting'] > 0 and r['coplanar'] > 0 and r['pairs_across_components'] == 0
    assert r['pairs_inside_component'] == r['intersecting'] + r['coplanar'] and r['nonmanifold_vertices'] == 0


def test_pierced_grid_one_large_triangle():
    v, f = M.pierced_grid(24)
    r = M.check(v, f)
    big = len(f) - 1
    assert r['report']['intersecting'] > 0 and r['report']['coplanar'] == 0
    assert (r['pairs'][:, 1] == big).all() and r['report']['pairs_inside_component'] == -1


def test_pseudonormal_sign_is_wrong_inside_a_self_intersecting_component():
    """the premise of --sign auto: at least 20 fixed queries where the pseudonormal of the nearest feature says outside and
    the exact winding number says inside, none of them near the surface or near |w| = 1/2"""
    v, f = M.ribbon_prism()
    mm = mesh_sdf_model.MeshModel(v, f)
    assert mm.closed and mm.components == 1 and not mm.inverted
    q = M.RIBBON_QUERIES
    assert len(q) >= 20
    d, det = mm.signed_distance(q, with_details=True)
    w = mesh_sdf_model.winding(q.astype(np.float64), mm.tri)
    assert not det['flagged'].any() and (np.abs(d) > 0.01).all()
    assert (np.abs(w - 1.0) < 1e-6).all()              # inside, by the exact sum
    assert (d < 0).all()                               # outside, says the pseudonormal of the nearest feature
