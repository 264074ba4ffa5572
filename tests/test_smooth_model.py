"""The numpy model of p2s_mesh_smooth (tests/smooth_model.py) on its own, with no device, against independent facts: the
closed form on a regular tetrahedron, a dense float64 evaluation of one half-step built another way, byte identity under
reordered faces, the classes of hand-made cases vertex by vertex, and what lambda | mu is for: a noisy sphere keeps its volume
under Taubin smoothing and loses it under Laplacian smoothing."""
import time

import numpy as np
import pytest

import smooth_model as SM


def test_tetrahedron_scales_by_the_closed_form():
    """every vertex of a regular tetrahedron centred at the origin has the other three as neighbours, whose mean is -p / 3: a
    half-step with w scales by 1 - 4 w / 3"""
    v, f = SM.tetrahedron()
    lam, mu = 0.5, -0.53
    k = (1 - 4 * lam / 3) * (1 - 4 * mu / 3)
    assert abs(k - 0.5688888888888889) < 1e-15
    m = SM.smooth(v, f, 1, lam, mu, 0)
    assert m['rc'] == 0 and m['cls'].tolist() == [0, 0, 0, 0] and m['report'][9] == 2
    ulp = np.spacing(np.float32(1.0))                                   # |coordinate| <= 1: one float32 ulp per half-step
    assert np.all(np.abs(m['verts'].astype(np.float64) - k * v.astype(np.float64)) <= 2 * ulp)
    one = SM.smooth(v, f, 1, lam, 0.0, 0)
    assert one['report'][9] == 1 and np.all(np.abs(one['verts'].astype(np.float64) - (1 - 4 * lam / 3) * v.astype(np.float64)) <= ulp)
    assert m['report'][10:11].view(np.float64)[0] == pytest.approx(3 * (1 - k) ** 2, rel=1e-6)


def _dense_half_step(v, f, w):
    """P + w (D^-1 A P - P) with a dense adjacency matrix filled face by face"""
    V = len(v)
    A = np.zeros((V, V))
    for a, b, c in np.asarray(f).tolist():
        A[a, b] = A[b, a] = A[b, c] = A[c, b] = A[a, c] = A[c, a] = 1.0
    P = v.astype(np.float64)
    return P + w * ((A @ P) / A.sum(axis=1)[:, None] - P)


@pytest.mark.parametrize('w', [0.5, -0.53, 1.0, -2.0])
def test_one_half_step_against_a_dense_evaluation(w):
    v, f = SM.icosphere(2, noise=0.05, seed=3)
    gv, gf = SM.grid(9, 7, noise=0.2, seed=4)
    for vv, ff in ((v, f), (gv, gf)):
        a, b, cnt = SM.edges(ff)
        cls = SM.classes(len(vv), a, b, cnt, 2)                         # mode free: every vertex moves, as in the dense form
        got = SM.half_step(vv, SM._blocks(*SM.rows(len(vv), a, b, cnt, cls)), w)
        want = _dense_half_step(vv, ff, w)
        assert got.dtype == np.float32 and not np.array_equal(got, vv)
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.float32(np.abs(want).max())))


def test_face_order_and_corner_order_change_no_byte():
    v, f = SM.grid(12, 9, noise=0.3, seed=1)
    for mode in (0, 1, 2):
        m = SM.smooth(v, f, 3, 0.5, -0.53, mode)
        for seed in (1, 2):
            g = SM.smooth(v, SM.shuffled(f, seed), 3, 0.5, -0.53, mode)
            assert g['verts'].tobytes() == m['verts'].tobytes() and g['cls'].tobytes() == m['cls'].tobytes()
            assert g['report'].tolist() == m['report'].tolist()
        assert not np.array_equal(m['verts'], v)


@pytest.mark.parametrize('name', sorted(SM.class_cases()))
def test_classes_by_hand(name):
    v, f, fixed, want = SM.class_cases()[name]
    for mode in (0, 1, 2):
        m = SM.smooth(v, f, 2, 0.5, -0.53, mode, fixed)
        assert m['cls'].tolist() == want[mode], (name, mode)
        assert m['report'][1:7].tolist() == np.bincount(want[mode], minlength=6).tolist()
        still = np.array(want[mode]) >= 2
        assert m['verts'][still].tobytes() == v[still].tobytes()
        if (~still).any():
            assert not np.any(np.all(m['verts'][~still] == v[~still], axis=1))


def test_a_curve_vertex_reads_its_two_boundary_neighbours_only():
    v, f = SM.grid(4, 4, noise=0.2, seed=2)
    a, b, cnt = SM.edges(f)
    cls = SM.classes(16, a, b, cnt, 1)
    start, col = SM.rows(16, a, b, cnt, cls)
    assert cls.reshape(4, 4).tolist() == [[1, 1, 1, 1], [1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1]]
    assert col[start[1]:start[2]].tolist() == [0, 2] and col[start[0]:start[1]].tolist() == [1, 4]      # an edge vertex; a corner
    assert col[start[5]:start[6]].tolist() == [0, 1, 4, 6, 9, 10]
    m = SM.smooth(v, f, 1, 0.5, 0.0, 1)
    want = v[1].astype(np.float64) + 0.5 * ((v[0].astype(np.float64) + v[2].astype(np.float64)) / 2.0 - v[1].astype(np.float64))
    assert m['verts'][1].tolist() == want.astype(np.float32).tolist() and m['report'][8] == 6


def test_taubin_keeps_the_volume_of_a_noisy_sphere_and_laplacian_does_not():
    v, f = SM.icosphere(3, noise=0.02, seed=7)
    assert len(v) == 642
    vol = SM.signed_volume(v, f)
    taubin = SM.signed_volume(SM.smooth(v, f, 10, 0.5, -0.53, 0)['verts'], f) / vol - 1
    laplace = SM.signed_volume(SM.smooth(v, f, 20, 0.5, 0.0, 0)['verts'], f) / vol - 1
    print('volume change: Taubin %+.2f %%, Laplacian %+.2f %%' % (100 * taubin, 100 * laplace))
    assert abs(taubin) < 0.03 and laplace < -0.15


def test_the_model_is_vectorised():
    v, f = SM.grid(200, 200, noise=0.2, seed=9)
    t0 = time.perf_counter()
    m = SM.smooth(v, f, 10, 0.5, -0.53, 0)
    dt = time.perf_counter() - t0
    print('40,000 vertices, 10 iterations: %.2f s' % dt)
    assert m['report'][1] == 198 * 198 and m['report'][3] == 4 * 199 and m['report'][9] == 20 and dt < 5.0


def test_overflow_is_counted():
    v, f = SM.tetrahedron()
    m = SM.smooth(v * np.float32(3e38), f, 1, 1.0, -2.0, 0)
    assert m['rc'] == SM.EINVAL and m['report'][11] > 0
