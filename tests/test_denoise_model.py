"""The numpy model of p2s_mesh_denoise (tests/denoise_model.py) alone, with no device: what the filter keeps, what it removes
on the noisy cube against Taubin smoothing, the classes by hand, dead faces, opposite orientations and the threshold's edge."""
import functools

import numpy as np
import pytest

import denoise_model as DM
import smooth_model as SM


@pytest.mark.parametrize('T', [0.0, 0.3, 0.5, 0.999])
def test_a_flat_grid_comes_back_byte_for_byte(T):
    v, f = DM.grid(9, 9)
    for mode in (0, 1):
        m = DM.denoise(v, f, T, 10, 10, mode)
        assert m['rc'] == 0 and m['verts'].tobytes() == v.tobytes()
        assert np.array_equal(m['normals'], np.tile(np.array([0, 0, 1], np.float32), (len(f), 1)))
        assert m['report'][10] == 0 and m['report'][8] == 10 and m['report'][9] == 10


def test_zero_iterations_come_back_byte_for_byte():
    v, f = DM.icosphere(2, noise=0.05, seed=3)
    v[5, 1] = -0.0
    geometric = DM.face_normals(v, f)
    for n_it, v_it in ((0, 0), (4, 0)):
        m = DM.denoise(v, f, 0.5, n_it, v_it, 1)
        assert m['verts'].tobytes() == v.tobytes() and m['report'][8:12].tolist() == [n_it, 0, 0, 0]
        assert (m['normals'].tobytes() == geometric.tobytes()) == (n_it == 0)
    m = DM.denoise(v, f, 0.5, 0, 3, 1)                                  # no normal iteration: the targets are the geometric normals
    assert m['normals'].tobytes() == geometric.tobytes() and m['verts'].tobytes() != v.tobytes()
    e = DM.denoise(v, f[:0], 0.5, 5, 5, 0)                              # no face
    assert e['verts'].tobytes() == v.tobytes() and e['cls'].tolist() == [3] * len(v) and e['report'][6:10].tolist() == [0, 0, 0, 0]


@functools.lru_cache(maxsize=None)
def cube_errors(n):
    v, f, clean = DM.noisy_cube(n)
    m = DM.denoise(v, f)
    taubin = SM.smooth(v, f, 10, 0.5, -0.53, 0)
    return (DM.normal_error_deg(v, f, clean), DM.normal_error_deg(taubin['verts'], f, clean), DM.normal_error_deg(m['verts'], f, clean), m)


@pytest.mark.parametrize('n', [12, 8])
def test_the_noisy_cube_keeps_its_edges(n):
    """the mean angle between the face normals and those of the clean cube.  A float64 prototype gave, at 12 x 12: input
    20.8, 10 Taubin iterations 9.8, this filter at its defaults 2.3 degrees; at 8 x 8: 22.2, 11.8 and 4.0."""
    noisy, taubin, filtered, m = cube_errors(n)
    print('cube %d x %d: noisy %.2f, taubin %.2f, denoised %.2f degrees' % (n, n, noisy, taubin, filtered))
    assert m['rc'] == 0 and m['report'][0] == (6 * n * n + 2) | (12 * n * n << 32) and m['report'][1] == 6 * n * n + 2
    assert noisy > 15.0
    assert filtered < 5.0 and filtered < 0.5 * taubin


CASES = DM.class_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_class_cases(name):
    v, f, fixed, want = CASES[name]
    for mode in (0, 1):
        m = DM.denoise(v, f, 0.5, 2, 2, mode, fixed)
        assert m['cls'].tolist() == want[mode]
        assert m['report'][1:6].tolist() == np.bincount(want[mode], minlength=5).tolist()
        still = m['cls'] != 0
        assert m['verts'][still].tobytes() == v[still].tobytes()
        if name == 'open_sheet':                                        # (a tetrahedron's faces do not see each other at T = 0.5)
            assert np.all(np.any(m['verts'][~still] != v[~still], axis=1))             # every free vertex of the sheet moves


def test_a_dead_face_stays_zero_and_moves_nobody():
    v, f, _, _ = CASES['dead_face_on_a_live_vertex']
    with_dead = DM.denoise(v, f, 0.2, 3, 3, 1)
    without = DM.denoise(v, f[:-1], 0.2, 3, 3, 1)
    assert with_dead['report'][6] == 1 and without['report'][6] == 0
    assert with_dead['normals'][-1].tolist() == [0, 0, 0] and with_dead['normals'][:-1].tobytes() == without['normals'].tobytes()
    assert with_dead['verts'].tobytes() == without['verts'].tobytes()
    assert with_dead['report'][7] == 5 and without['report'][7] == 4                   # the dead face is still a neighbour


def test_opposite_sheets_on_the_same_vertices_do_not_mix():
    v, f = DM.grid(5, 5, noise=0.15, seed=2)
    back = f[:, [0, 2, 1]]
    one = DM.denoise(v, f, 0.0, 4, 0, 1)
    two = DM.denoise(v, np.concatenate([f, back]), 0.0, 4, 0, 1)
    F = len(f)
    # a face and its twin have d = -1; two faces that make less than a right angle on one sheet make more than one across
    assert two['normals'][:F].tobytes() == one['normals'].tobytes()
    assert two['normals'][F:].tobytes() == (-one['normals']).tobytes()
    assert two['report'][7] == 2 * one['report'][7]


def test_d_equal_to_the_threshold_contributes_nothing():
    """two faces at a right angle, T = 0: d is exactly 0, which is not above T, so either normal stays"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1]], np.int32)                      # normals (0, 0, 1) and (0, 1, 0)
    m = DM.denoise(v, f, 0.0, 5, 0, 1)
    assert m['normals'].tolist() == [[0, 0, 1], [0, 1, 0]] and m['report'][7] == 2
    tilted = v.copy()
    tilted[3] = [0, -0.5, 1]                                            # normal (0, 1, 0.5): less than a right angle, they mix
    m = DM.denoise(tilted, f, 0.0, 1, 0, 1)
    assert m['normals'][0, 1] > 0 and m['normals'][0, 2] < 1
