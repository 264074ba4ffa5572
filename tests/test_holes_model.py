"""The numpy model of p2s_mesh_fill_holes (tests/holes_model.py) on its own, with no device: the minimum-area triangulation
against the fan of p2s_mesh_repair on an L-shaped hole, the tie rule, the dynamic programme against every triangulation of
small loops, and the guarantees of rule f by brute force on every small case."""
import math

import numpy as np
import pytest

import holes_model as HM

SMALL = HM.small_cases()


def _p(points):
    return np.asarray(points, np.float64).tolist()


def test_l_hexagon_has_area_3_from_every_start_and_the_fan_has_not():
    fans = []
    for r in range(6):
        p = _p(HM.rotated(HM.L_HEXAGON, r))
        total, lam = HM.triangulate(p)
        assert total == 3.0
        assert sum(HM.area(p, i, k, j) for i, j, k in HM.emit(lam, 6)) == 3.0
        fans.append(HM.fan_area(p))
        v, f, K = SMALL['l_hexagon_%d' % r]
        m = HM.fill(v, f, K)
        assert m['hole_area'].tolist() == [3.0] and m['holes'].tolist() == [[0, 6, len(f), HM.FILLED]]
    assert sorted(fans) == [3.0, 3.0, 4.0, 4.0, 4.0, 4.0]


def test_the_tie_rule_alone_fixes_a_convex_planar_polygon():
    p = _p(HM.CONVEX)
    n = len(p)
    total, lam = HM.triangulate(p)
    every = {sum(HM.area(p, i, k, j) for i, k, j in t) for t in HM.all_triangulations(0, n - 1)}
    assert every == {total}                               # integer corners: every triangulation has exactly the same area
    # the smallest k everywhere: the fan from the LAST vertex, (i, n - 1) split at i + 1
    assert HM.emit(lam, n) == [(i, n - 1, i + 1) for i in range(n - 2)]


@pytest.mark.parametrize('n', [3, 4, 5, 6, 7])
def test_dp_against_every_triangulation(n):
    rng = np.random.default_rng(n)
    for trial in range(6):
        p = _p(HM.random_loop(n, rng))
        forbidden = [] if trial < 3 or n < 5 else [(1, 3)]
        total, lam = HM.triangulate(p, forbidden)
        best = math.inf
        for t in HM.all_triangulations(0, n - 1):
            if any((i, j) in forbidden or (i, k) in forbidden or (k, j) in forbidden for i, k, j in t):
                continue
            best = min(best, sum(HM.area(p, i, k, j) for i, k, j in t))
        got = HM.emit(lam, n)
        assert len(got) == n - 2 and math.isclose(total, best, rel_tol=1e-14)
        assert math.isclose(sum(HM.area(p, i, k, j) for i, j, k in got), total, rel_tol=1e-14)
        assert not any((min(a, b), max(a, b)) in forbidden for i, j, k in got for a, b in ((i, j), (i, k), (k, j)))


@pytest.mark.parametrize('name', sorted(SMALL))
def test_guarantees_on_every_small_case(name):
    v, f, K = SMALL[name]
    m = HM.fill(v, f, K)
    HM.check_guarantees(v, f, m, K)
    rep = m['report']
    assert rep[1] == len(f) + rep[4] and rep[2] == len(m['holes']) == rep[3] + rep[5] + rep[6]
    assert rep[4] == sum(n - 2 for _, n, _, why in m['holes'].tolist() if why == HM.FILLED)
    assert rep[8] == rep[7] - sum(n for _, n, _, why in m['holes'].tolist() if why == HM.FILLED)
    assert np.array_equal(m['faces'][:len(f)], f) and np.all(m['face_src'][len(f):] == -1)


def test_what_the_named_cases_are_about():
    rep = lambda name: HM.fill(*SMALL[name])['report'].tolist()
    v, f, K = SMALL['best_chord_exists']
    free = HM.fill(v[:-2], f[:-4], K)
    taken = HM.fill(v, f, K)
    assert taken['report'][3] == 1 and taken['hole_area'][0] > free['hole_area'][0] and taken['report'][11] == 0
    assert rep('one_chord_exists')[1:7] == [4, 1, 1, 2, 0, 0] and rep('one_chord_exists')[8] == 0      # a closed tetrahedron
    assert HM.fill(*SMALL['one_chord_exists'])['faces'][2:].tolist() == [[0, 3, 1], [1, 3, 2]]
    assert rep('both_chords_exist')[2:7] == [1, 0, 0, 0, 1] and HM.fill(*SMALL['both_chords_exist'])['holes'][0].tolist() == [0, 4, -1, 2]
    assert rep('two_loops_meet')[2:10] == [0, 0, 0, 0, 0, 11, 11, 1]
    assert rep('flipped_neighbour')[2:4] == [0, 0] and rep('flipped_neighbour')[9] == 1
    assert rep('closed')[1:10] == [8, 0, 0, 0, 0, 0, 0, 0, 0] and rep('no_faces') == [4] + [0] * 15
    assert rep('a_copy')[1:10] == [len(SMALL['a_copy'][1]), 3, 0, 0, 3, 0, 22, 22, 3]
    assert rep('limit_7')[2:7] == [3, 2, 6, 1, 0] and rep('limit_7')[10] == 7
    assert HM.fill(*SMALL['loop3'])['faces'][-1].tolist() == [0, 2, 1]          # the face the fan of p2s_mesh_repair writes


def test_the_sphere_has_six_holes_of_3_to_60_edges():
    v, closed, g = HM.sphere_with_holes()
    assert HM.boundary(closed) == []
    sizes = sorted(len(loop) for loop in HM.loops(g, len(v)))
    assert len(sizes) == 6 and sizes[0] == 3 and 30 < sizes[-1] <= 60 and sum(sizes) == len(HM.boundary(g))
    m = HM.fill(v, g, 60)
    assert m['report'][3] == 6 and m['report'][8] == 0
