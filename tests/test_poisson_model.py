"""The float64 model of the Screened Poisson baseline (tests/poisson_model.py) against properties of its definition
(DESIGN 4.8 f10).  No device."""
import numpy as np
import pytest

import poisson_model as P


@pytest.fixture(scope='module')
def sphere():
    return P.sphere()


def test_matrix_is_symmetric_positive_definite_at_depth_3(sphere):
    pts, nrm = sphere
    lev = P.Level(pts[:2000], nrm[:2000], 3)
    A = lev.A.toarray()
    assert np.array_equal(A, A.T) or np.abs(A - A.T).max() <= 1e-15 * np.abs(A).max()
    ev = np.linalg.eigvalsh((A + A.T) / 2.0)
    print('eigenvalues', ev.min(), ev.max())
    assert ev.min() > 0.0
    # without the screen the operator has the constants in its null space: the screen is what makes it definite
    ev0 = np.linalg.eigvalsh(lev.A0.toarray())
    assert abs(ev0.min()) <= 1e-12 * ev0.max()


def test_rhs_of_one_point_written_out_by_hand():
    """one point with a unit normal (a second one far away spans the box): b at every node from the 1-D entries and the
    point's 8 weights, no Kronecker product"""
    pts = np.array([[0.30, 0.41, 0.52], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], np.float32)
    nrm = np.array([[0.0, 0.6, 0.8], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    lev = P.Level(pts, nrm, 3, scale=1.0)
    R, h = lev.R, lev.h
    c, t = P.cells(pts[:1], lev.lo, h, R)
    c, t = c[0], t[0]
    nv = -nrm[0].astype(np.float64) * lev.a / h ** 3
    want = np.zeros((R, R, R))
    for k in range(8):
        kx, ky, kz = k >> 2, (k >> 1) & 1, k & 1
        w = (t[0] if kx else 1 - t[0]) * (t[1] if ky else 1 - t[1]) * (t[2] if kz else 1 - t[2])
        ni, nj, nk = c[0] + kx, c[1] + ky, c[2] + kz
        for i in range(max(ni - 1, 0), min(ni + 2, R)):
            for j in range(max(nj - 1, 0), min(nj + 2, R)):
                for q in range(max(nk - 1, 0), min(nk + 2, R)):
                    want[i, j, q] += w * (nv[0] * P.g1(i, ni, R, h) * P.m1(j, nj, R, h) * P.m1(q, nk, R, h) +
                                          nv[1] * P.m1(i, ni, R, h) * P.g1(j, nj, R, h) * P.m1(q, nk, R, h) +
                                          nv[2] * P.m1(i, ni, R, h) * P.m1(j, nj, R, h) * P.g1(q, nk, R, h))
    got = lev.b.reshape(R, R, R)
    assert lev.n_occ == 3 and np.abs(want).max() > 0
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize('depth', [4, 5])
def test_sphere_is_recovered_within_half_a_cell(sphere, depth):
    pts, nrm = sphere
    chi, lev, iters = P.solve(pts, nrm, depth)
    vol, iso = P.volume(lev, chi)
    u = np.random.default_rng(1).standard_normal((2000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    centre = lev.lo + lev.h * (lev.R - 1) / 2.0
    r = P.ray_crossings(vol, lev.lo, lev.h, lev.R, centre, u, 0.5 * lev.h * (lev.R - 1))
    # the crossing is measured from the box centre; the sphere's own centre is the origin
    hit = centre + r[:, None] * u
    err = np.abs(np.linalg.norm(hit, axis=1) - 0.5) / lev.h
    print('depth', depth, 'iterations', iters, 'iso', iso, 'max error / h', np.nanmax(err))
    assert np.isfinite(r).all() and err.max() <= 0.5


def test_border_rule_leaves_no_positive_border_node(sphere):
    pts, nrm = sphere
    lev = P.Level(pts, nrm, 3)
    chi = np.random.default_rng(2).standard_normal(lev.R ** 3)
    vol, _ = P.volume(lev, chi)
    m = P.border_mask(lev.R)
    assert m.sum() == lev.R ** 3 - (lev.R - 2) ** 3
    assert (vol[m] <= 0).all() and (vol[~m] > 0).any()
    assert np.array_equal(np.abs(vol), np.abs((chi.reshape(vol.shape) - P.iso_value(lev, chi)).astype(np.float32)))
