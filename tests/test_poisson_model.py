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


FREE_CASES = {k: v for k, v in P.piece_cases().items() if k in ('sphere', 'on_node_scale1', 'dense_cell')}
# The two levels form every node's value from the same terms, in another order and with other intermediate products.  The
# longest chain is the screen term of a node of the dense cell: its row of W^T holds L <= 400 entries (asserted).  Level
# sums L products into each entry of W^T W (2 L roundings) and then 27 products of the row of A (54); FreeLevel sums 8
# products into u (16) and L products along the row (2 L).  The stencil part adds 27 terms of three rounded factors on one
# side and three nested 3-term sums on the other: below 100 on either.  4 L + 170 <= 1770 roundings of 2^-53 = 2e-13 if all
# pointed one way and every term were as large as the sum; half of that, 1e-13, still leaves what is measured (printed:
# below 1e-14 everywhere) two orders away, and a wrong coefficient or a shifted slice is an error of order 1.
FREE_TOL, FREE_MAX_ROW = 1e-13, 400


@pytest.mark.parametrize('depth', [3, 4, 5])
@pytest.mark.parametrize('case', sorted(FREE_CASES))
def test_matrix_free_level_is_the_sparse_level(case, depth):
    """every field of FreeLevel, apply and apply_abs (x seeded random and x = 1) against Level: the integers and the box
    exactly, the vectors node by node within 1e-13 * (the sum over absolute values of the node's terms)"""
    pts, nrm, scale = FREE_CASES[case]
    ref, lev = P.Level(pts, nrm, depth, scale=scale), P.FreeLevel(pts, nrm, depth, scale=scale)
    assert np.diff(lev.Wt.indptr).max() <= FREE_MAX_ROW
    assert lev.n_occ == ref.n_occ and lev.R == ref.R and lev.h == ref.h and np.array_equal(lev.lo, ref.lo)
    assert lev.a == ref.a and lev.lam == ref.lam
    assert (lev.W != ref.W).nnz == 0 and (lev.W64 != ref.W).nnz == 0
    x = np.random.default_rng(11).standard_normal(lev.R ** 3)
    one = np.ones(lev.R ** 3)
    for name, got, want, mag in (('v', lev.v, ref.v, ref.v_abs), ('v_abs', lev.v_abs, ref.v_abs, ref.v_abs),
                                 ('b', lev.b, ref.b, ref.b_abs), ('b_abs', lev.b_abs, ref.b_abs, ref.b_abs),
                                 ('diag', lev.diag, ref.diag, ref.diag),
                                 ('A x', lev.apply(x), ref.apply(x), ref.apply_abs(x)),
                                 ('|A| |x|', lev.apply_abs(x), ref.apply_abs(x), ref.apply_abs(x)),
                                 ('A 1', lev.apply(one), ref.apply(one), ref.apply_abs(one)),
                                 ('|A| 1', lev.apply_abs(one), ref.apply_abs(one), ref.apply_abs(one))):
        assert got.shape == want.shape
        err = np.abs(got - want)
        print(case, depth, name, 'worst err / magnitude', np.max(err / np.maximum(mag, 1e-300)))
        assert np.abs(want).max() > 0 and (err <= FREE_TOL * mag).all(), name


@pytest.mark.parametrize('Rc', [2, 5, 9])
def test_matrix_free_prolongation_is_the_matrix(Rc):
    x = np.random.default_rng(4).standard_normal(Rc ** 3)
    want = P.prolong_matrix(Rc) @ x
    assert np.abs(P.prolong(x, Rc) - want).max() <= 4 * 2.0 ** -53 * np.abs(x).max()      # 7 additions, 3 exact halvings
    assert np.abs(P.prolong(x, Rc, odd_weight=0.25) - want).max() > 0.1


def test_one_step_cascade_written_out_with_the_sparse_level(sphere):
    """the float64 cascade of one CG step per level against the same steps with Level's A and prolong_matrix"""
    pts, nrm = sphere[0][:2000], sphere[1][:2000]
    x = None
    for d in (3, 4):
        lev = P.Level(pts, nrm, d)
        x0 = np.zeros(lev.R ** 3) if x is None else P.prolong_matrix((lev.R + 1) // 2) @ x
        r = lev.b - lev.A @ x0
        z = r / lev.diag
        x = x0 + (r @ z) / (z @ (lev.A @ z)) * z
    got, flev = P.one_step_cascade(pts, nrm, 4)
    assert flev.R == 17 and np.abs(x).max() > 0
    assert np.abs(got - x).max() <= 1e-12 * np.abs(x).max()


ONE_STEP_MARGIN = 4.0      # the device within 4 d32 of the float64 cascade (tests/test_gpu_poisson.py)


def test_one_step_cascade_notices_a_wrong_prolongation(sphere):
    """The device test holds the device's one-step cascade within 4 d32 of the float64 one, d32 = the distance of the
    float32-store emulation.  That has teeth only if a wrong prolongation lies further away: half the weight on the odd
    nodes (per axis 0.25 instead of 0.5), depth 5, the 20000-point sphere."""
    pts, nrm = sphere
    c64, _ = P.one_step_cascade(pts, nrm, 5)
    c32, _ = P.one_step_cascade(pts, nrm, 5, np.float32)
    bad, _ = P.one_step_cascade(pts, nrm, 5, odd_weight=0.25)
    d32, d_bad = np.abs(c32 - c64).max(), np.abs(bad - c64).max()
    print('max |chi|', np.abs(c64).max(), 'd32', d32, 'wrong prolongation', d_bad, 'factor over 4 d32', d_bad / (ONE_STEP_MARGIN * d32))
    assert d32 > 0 and d_bad > ONE_STEP_MARGIN * d32


def test_border_rule_leaves_no_positive_border_node(sphere):
    pts, nrm = sphere
    lev = P.Level(pts, nrm, 3)
    chi = np.random.default_rng(2).standard_normal(lev.R ** 3)
    vol, _ = P.volume(lev, chi)
    m = P.border_mask(lev.R)
    assert m.sum() == lev.R ** 3 - (lev.R - 2) ** 3
    assert (vol[m] <= 0).all() and (vol[~m] > 0).any()
    assert np.array_equal(np.abs(vol), np.abs((chi.reshape(vol.shape) - P.iso_value(lev, chi)).astype(np.float32)))
