"""The numpy model of p2s_mesh_manifold (tests/manifold_model.py) against its own independent checker, on every case and every
mode: the guarantee of rule f, idempotence, the source arrays, copied coordinates, the report's arithmetic; and the expected
results of the hand-made cases."""
import functools

import numpy as np
import pytest

import manifold_model as MM

CASES = MM.small_cases()
HAND = sorted(k for k in CASES if not k.startswith('soup'))


@functools.lru_cache(maxsize=None)
def big():
    return MM.big_case()


def check(v, f, mode):
    m = MM.manifold(v, f, mode)
    V, F = len(v), len(f)
    rep = m['report']
    V1, F1 = len(m['verts']), len(m['faces'])
    # the guarantee
    edges, vertices = MM.defects(m['faces'])
    assert edges == 0
    if mode & 2:
        assert vertices == 0
    # idempotence: the same bytes from a second call
    again = MM.manifold(m['verts'], m['faces'], mode)
    assert again['verts'].tobytes() == m['verts'].tobytes() and np.array_equal(again['faces'], m['faces'])
    assert again['report'][3] == 0 and again['report'][4] == 0 and again['report'][5] == 0 and again['report'][6] == 0
    # the source arrays; coordinates copied bit for bit; order and winding
    assert m['verts'].dtype == np.float32 and m['verts'].tobytes() == np.asarray(v, np.float32)[m['vert_src']].tobytes()
    assert np.array_equal(m['vert_src'][m['faces']], np.asarray(f)[m['face_src']])
    assert np.all(np.diff(m['face_src']) > 0) and np.all(np.diff(m['vert_src']) >= 0)
    if F1:
        assert np.array_equal(np.unique(m['faces']), np.arange(V1))             # every output vertex is referenced
        first = np.full(V1, F1)
        np.minimum.at(first, m['faces'].reshape(-1), np.repeat(np.arange(F1), 3))
        same = np.diff(m['vert_src']) == 0
        assert np.all(np.diff(first)[same] > 0)                                  # classes of one vertex by their smallest face
    # the report's arithmetic
    referenced = np.unique(np.asarray(f)[m['face_src']]).size
    assert rep[0] == V | (F << 32) and rep[1] == V1 and rep[2] == F1 and rep[4] == F - F1
    assert rep[1] - rep[6] == referenced and rep[1] - rep[6] + rep[7] == V
    assert rep[5] <= rep[6] and (rep[5] == 0) == (rep[6] == 0) and np.all(rep[11:] == 0)
    assert rep[3] == MM.defects(f)[0]
    if not mode & 1:
        assert rep[4] == 0
    if not mode & 2:
        assert rep[5] == 0 and rep[6] == 0 and rep[10] <= rep[3]
    if rep[3] == 0:
        assert rep[4] == 0 and rep[10] == 0 and rep[9] == rep[8]
    if mode == 2:
        assert 3 * F1 == 2 * (len(MM.edge_faces(m['faces'])) - rep[9]) + rep[9]   # every output edge has one or two faces
    return m


@pytest.mark.parametrize('mode', MM.MODES)
@pytest.mark.parametrize('name', HAND)
def test_hand_made_cases(name, mode):
    check(*CASES[name], mode)


@pytest.mark.parametrize('mode', MM.MODES)
def test_random_soups(mode):
    edges = vertices = 0
    for name in sorted(CASES):
        if name.startswith('soup'):
            v, f = CASES[name]
            d = MM.defects(f)
            edges, vertices = edges + d[0], vertices + d[1]
            check(v, f, mode)
    assert edges > 500 and vertices > 500                   # the soups do hold what the unit repairs


@pytest.mark.parametrize('mode', MM.MODES)
def test_big_case(mode):
    v, f = big()
    assert len(f) == 39600
    m = check(v, f, mode)
    assert m['report'][3] == 66 + 5 and MM.defects(f)[1] > 66
    assert (m['report'][4] > 0) == bool(mode & 1) and (m['report'][5] > 66) == bool(mode & 2)


def test_expected_results():
    r = lambda name, mode: MM.manifold(*CASES[name], mode)
    # two tetrahedra sharing an edge: two closed tetrahedra of 8 vertices, one rejoined edge each
    m = r('tetras_sharing_an_edge', 2)
    assert m['report'][1:11].tolist() == [8, 8, 1, 0, 2, 2, 2, 0, 0, 2] and MM.defects(m['faces']) == (0, 0)
    assert m['vert_src'].tolist() == [0, 0, 1, 1, 2, 3, 6, 7]                     # 4 and 5 are the second one's 0 and 1, unreferenced
    # ... sharing a vertex: the vertex doubles
    m = r('tetras_sharing_a_vertex', 2)
    assert m['report'][1:11].tolist() == [8, 8, 0, 0, 1, 1, 1, 0, 0, 0]
    assert r('tetras_sharing_a_vertex', 1)['report'][1:11].tolist() == [7, 8, 0, 0, 0, 0, 1, 0, 0, 0]
    # a closed mesh comes back as it is
    m = r('tetra', 3)
    assert m['verts'].tobytes() == CASES['tetra'][0].tobytes() and np.array_equal(m['faces'], CASES['tetra'][1])
    # the book: the two largest pages stay (mode 1); every page gets its own spine (mode 2)
    m = r('book4', 1)
    assert m['face_src'].tolist() == [2, 3] and m['report'][1:11].tolist() == [4, 2, 1, 2, 0, 0, 2, 8, 4, 1]
    m = r('book4', 2)
    assert m['report'][1:11].tolist() == [12, 4, 1, 0, 2, 6, 0, 8, 12, 0]
    # equal q: the tie goes to the smaller face id
    assert r('equal_q', 1)['face_src'].tolist() == [0, 1] and r('equal_q_four', 1)['face_src'].tolist() == [0, 3]
    assert r('duplicate_faces_on_an_edge', 1)['face_src'].tolist() == [0, 1]          # 0 and 2, the same vertex set: q equal
    m = r('duplicate_faces', 3)
    assert np.array_equal(m['faces'], CASES['duplicate_faces'][1]) and m['report'][1:11].tolist() == [3, 2, 0, 0, 0, 0, 0, 0, 0, 0]
    # the over-removal of rule b
    m = r('over_removal', 1)
    assert m['face_src'].tolist() == [1, 2, 3] and m['report'][1:11].tolist() == [6, 3, 2, 2, 0, 0, 1, 9, 7, 1]
    # unreferenced vertices go, wherever they are
    m = r('unreferenced_vertices', 2)
    assert m['report'][7] == 4 and m['vert_src'].tolist() == [1, 1, 1, 2, 2, 2, 3, 6, 7]
    # the two fans: the apex doubles, nothing else
    v, f = CASES['two_fans']
    m = MM.manifold(v, f, 2)
    assert m['report'][1:11].tolist() == [172, 170, 0, 0, 1, 1, 0, 170, 170, 0]
    # octahedra sharing the chain 0 - 1 - 2: the middle vertex gets four classes, the ends two; the four faces of a shared edge part
    assert r('octahedra_sharing_two_edges', 2)['report'][1:11].tolist() == [14, 16, 2, 0, 3, 5, 3, 0, 8, 0]
    # the empty results
    for name in ('empty', 'vertices_only'):
        m = r(name, 3)
        assert m['verts'].shape == (0, 3) and m['faces'].shape == (0, 3) and m['report'][7] == len(CASES[name][0])


def test_invalid_input_is_refused():
    v, f = CASES['book3']
    for bad in (np.array([[0, 1, 5]]), np.array([[0, -1, 2]]), np.array([[0, 1, 1]]), np.array([[2, 1, 2]])):
        with pytest.raises(ValueError):
            MM.manifold(v, bad, 2)
    nan = v.copy()
    nan[1, 1] = np.inf
    with pytest.raises(ValueError):
        MM.manifold(nan, f, 2)
    with pytest.raises(ValueError):
        MM.manifold(v, f, 0)
