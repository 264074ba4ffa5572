"""The Screened Poisson baseline on the device (points2surf_amd.poisson: p2s_poisson_system, p2s_poisson_reconstruct)
against its float64 model (tests/poisson_model.py): the pieces of one level node by node within a rounding bound, the
solve by its residual in the model's A and b, the surface, an open scan, determinism, refusals and capacities; the same
at the depths and point counts at which the kernels' grids are capped and stride (matrix-free model), one CG step per level
against the model's cascade, levels that stop unconverged."""
import ctypes

import numpy as np
import pytest
import torch

import poisson_model as P

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# Roundings on the longest path from an input to an output of the device's float32 pieces (csrc/p2s_poisson.hip); every sum
# over points is float64 (2^-53 per term: nothing against these).  The bound of a sum evaluated in any order is
# (number of roundings on its longest path) * 2^-24 * (the same sum over absolute values); one more for the second order.
#   b:    v = one weight rounding + one rounding of the float64 node sum (2); three factors, each a coefficient rounding,
#         a product and two additions (12); two additions join the three terms (2)                             -> 16 + 1
#   A x:  three factors as above (12), one addition joins (s m + m s) x along axis 1 and one the two halves along axis 0 (2),
#         the screen term is added once (1); its own branch is shorter: weight, u = W x rounded, weight, that addition (4)  -> 15 + 1
#   diag: three rounded coefficients, two products (5), two additions (2), the screen term added once (1)      ->  8 + 1
C_B, C_AX, C_DIAG = 17, 16, 9


def _cases():
    return P.piece_cases()


CASES = _cases()


@pytest.mark.parametrize('depth', [3, 4])
@pytest.mark.parametrize('case', sorted(CASES))
def test_pieces_against_the_model(case, depth):
    """b, A x (x seeded random and x = 1) and diag(A) node by node within c * 2^-24 * (the sum over absolute values)"""
    from points2surf_amd import poisson
    pts, nrm, scale = CASES[case]
    lev = P.Level(pts, nrm, depth, scale=scale)
    x = np.random.default_rng(11).standard_normal(lev.R ** 3).astype(np.float32)
    b, diag, ax, rep = poisson.system(pts, nrm, depth, x=x, scale=scale)
    _, _, ax1, _ = poisson.system(pts, nrm, depth, x=np.ones(lev.R ** 3, np.float32), scale=scale)
    lv = rep['levels'][0]
    assert lv['n_occ'] == lev.n_occ
    assert abs(lv['lam'] - lev.lam) <= 1e-6 * lev.lam and abs(rep['h'] - lev.h) <= 1e-6 * lev.h
    assert np.abs(np.array(rep['lo']) - lev.lo).max() <= 1e-6 * np.abs(lev.lo).max()
    for name, got, want, mag, c in (('b', b, lev.b, lev.b_abs, C_B), ('diag', diag, lev.diag, lev.diag, C_DIAG),
                                    ('A x', ax, lev.apply(x), lev.apply_abs(x), C_AX),
                                    ('A 1', ax1, lev.apply(np.ones(lev.R ** 3)), lev.apply_abs(np.ones(lev.R ** 3)), C_AX)):
        err = np.abs(got.cpu().numpy().astype(np.float64).reshape(-1) - want)
        bound = c * U * mag
        worst = np.max(err / np.maximum(bound, 1e-300))
        print(case, depth, name, 'max |want|', np.abs(want).max(), 'max err', err.max(), 'worst err / bound', worst)
        assert np.abs(want).max() > 0 and (err <= bound).all(), (name, worst)


# Mirror of the launch constants of csrc/p2s_poisson.hip (PS_TX, PS_TY, PS_TZ, PS_MAX_PART, PS_CHECK_EVERY; 256 threads per
# workgroup).  The tests below assert from them, on the model's side, that their input reaches the branch they are about.
PS_TX, PS_TY, PS_TZ, PS_MAX_PART, PS_CHECK_EVERY, PS_THREADS = 8, 8, 32, 1024, 8, 256


def _ceil(a, b):
    return -(-a // b)


def _launch(lev, n):
    """the launch shapes of one level as ps_level_setup forms them, and the rows of W^T (the active nodes)"""
    R = lev.R
    tiles_z = _ceil(R, PS_TZ)
    return dict(tiles_z=tiles_z, tail_z=R - (tiles_z - 1) * PS_TZ, n_tiles=_ceil(R, PS_TX) * _ceil(R, PS_TY) * tiles_z,
                g_screen_wanted=_ceil(8 * n, PS_THREADS), g_screen=min(_ceil(8 * n, PS_THREADS), PS_MAX_PART),
                g_vec_wanted=_ceil(R ** 3, 4 * PS_THREADS), rows=int(np.unique(lev.W.indices).size),
                g_points_wanted=_ceil(n, PS_THREADS))


def _more_cases():
    rng = np.random.default_rng(7)
    out = {'sphere': CASES['sphere'], 'on_node_scale1': CASES['on_node_scale1']}
    # few points far apart: about 8 active nodes per point, so more rows of W^T than one pass of ps_screen_kernel takes
    out['scatter40'] = (rng.random((40, 3)).astype(np.float32), rng.standard_normal((40, 3)).astype(np.float32), 1.1)
    out['sphere40k'] = P.sphere(40000, 3) + (1.1,)
    # more points than ps_validate_kernel's and ps_iso_kernel's grids take in one pass: a sphere of radius 0.25 around the
    # centre of the unit cube; the cube's two corners come last, in the strided part, they alone fix the box and with
    # scale 1.0 sit on the first and the last node
    node_pts, node_nrm, _ = CASES['on_node_scale1']
    pts, nrm = P.sphere(263000 - 2, 6, radius=0.25)
    out['many_points'] = (np.concatenate([pts + np.float32(0.5), node_pts[1:]]), np.concatenate([nrm, node_nrm[1:]]), 1.0)
    return out


MORE = _more_cases()
_FREE = {}


def _free(case, depth):
    """the matrix-free float64 level of a case, made once"""
    if (case, depth) not in _FREE:
        pts, nrm, scale = MORE[case]
        _FREE[case, depth] = P.FreeLevel(pts, nrm, depth, scale=scale)
    return _FREE[case, depth]


def _check_pieces(case, depth, with_ax=True):
    """the assertion of test_pieces_against_the_model on the matrix-free level; every node is compared"""
    from points2surf_amd import poisson
    pts, nrm, scale = MORE[case]
    lev = _free(case, depth)
    if with_ax:
        x = np.random.default_rng(11).standard_normal(lev.R ** 3).astype(np.float32)
        one = np.ones(lev.R ** 3, np.float32)
        b, diag, ax, rep = poisson.system(pts, nrm, depth, x=x, scale=scale)
        _, _, ax1, _ = poisson.system(pts, nrm, depth, x=one, scale=scale)
    else:
        b, diag, _, rep = poisson.system(pts, nrm, depth, scale=scale)
    lv = rep['levels'][0]
    assert lv['n_occ'] == lev.n_occ
    assert abs(lv['lam'] - lev.lam) <= 1e-6 * lev.lam and abs(rep['h'] - lev.h) <= 1e-6 * lev.h
    assert np.abs(np.array(rep['lo']) - lev.lo).max() <= 1e-6 * np.abs(lev.lo).max()
    pieces = [('b', b, lev.b, lev.b_abs, C_B), ('diag', diag, lev.diag, lev.diag, C_DIAG)]
    if with_ax:
        pieces += [('A x', ax, lev.apply(x), lev.apply_abs(x), C_AX), ('A 1', ax1, lev.apply(one), lev.apply_abs(one), C_AX)]
    for name, got, want, mag, c in pieces:
        err = np.abs(got.cpu().numpy().astype(np.float64).reshape(-1) - want)
        bound = c * U * mag
        worst = np.max(err / np.maximum(bound, 1e-300))
        print(case, depth, name, 'max |want|', np.abs(want).max(), 'max err', err.max(), 'worst err / bound', worst)
        assert np.abs(want).max() > 0 and (err <= bound).all(), (name, worst)


@pytest.mark.parametrize('depth', [5, 6])
def test_pieces_across_the_stencil_tiles_of_axis_2(depth):
    """ps_stencil_kernel with two (R = 33) and three (R = 65) tiles along axis 2, the last of one node: the halo read across
    a z-tile edge from the neighbouring tile's nodes, the tail tile's 31 idle lanes"""
    shape = _launch(_free('sphere', depth), 2000)
    assert shape['tiles_z'] == depth - 3 and shape['tail_z'] == 1
    _check_pieces('sphere', depth)


@pytest.mark.parametrize('depth', [3, 4, 5])
def test_pieces_with_more_rows_than_one_screen_pass(depth):
    """ps_screen_kernel's later passes (r0 += gridDim.x * 32): 40 points launch 2 workgroups of 32 rows, their 8 * 40 = 320
    entries fall on 255 to 320 distinct nodes"""
    shape = _launch(_free('scatter40', depth), 40)
    print(shape)
    assert shape['g_screen'] == shape['g_screen_wanted'] and shape['rows'] > 2 * 32 * shape['g_screen']
    _check_pieces('scatter40', depth)


def test_pieces_at_depth_7():
    """R = 129, 40000 points: ps_stencil_kernel strides over more tiles than workgroups (tile += gridDim.x, the barrier at
    the loop head, the dot product carried over tiles) with 5 tiles along axis 2; ps_screen_kernel's grid is capped at
    PS_MAX_PART and takes 3 passes"""
    shape = _launch(_free('sphere40k', 7), 40000)
    print(shape)
    assert shape['n_tiles'] > PS_MAX_PART and shape['tiles_z'] == 5 and shape['tail_z'] == 1
    assert shape['g_screen_wanted'] > PS_MAX_PART and shape['rows'] > 2 * 32 * shape['g_screen']
    _check_pieces('sphere40k', 7)


def test_pieces_of_more_points_than_one_validate_pass():
    """263000 points at depth 3: ps_validate_kernel's grid is capped at PS_MAX_PART workgroups and strides, the two points
    that fix the box lie in the strided part: lo, h, n_occ, lambda, b and diag"""
    lev = _free('many_points', 3)
    shape = _launch(lev, 263000)
    assert MORE['many_points'][0].shape[0] == 263000 and shape['g_points_wanted'] > PS_MAX_PART
    assert 263000 - 2 >= PS_MAX_PART * PS_THREADS                             # both corners are read by a second pass
    inner = MORE['many_points'][0][:-2]
    assert inner.min() > 0.2 and inner.max() < 0.8                             # the box is the two last points' alone
    assert np.array_equal(lev.lo, [0.0, 0.0, 0.0]) and lev.h == 0.125
    _check_pieces('many_points', 3, with_ax=False)


@pytest.fixture(scope='module')
def sphere():
    return P.sphere()


@pytest.fixture(scope='module')
def model(sphere):
    """the model's solutions of the sphere, depth -> (chi, Level)"""
    out = {}
    for depth in (4, 5):
        chi, lev, _ = P.solve(sphere[0], sphere[1], depth)
        out[depth] = (chi, lev)
    return out


CG_TOL, MAX_ITERS = 1e-3, 500


def _check_reported_residual(rep, true):
    """the finest level's reported residual against the one computed in the model's system"""
    fine = rep['levels'][-1]
    print('finest level: reported residual', fine['residual'], 'true', true, 'iterations', [lv['iterations'] for lv in rep['levels']])
    if fine['iterations'] < MAX_ITERS:
        assert fine['residual'] <= CG_TOL
    assert abs(true - fine['residual']) <= CG_TOL


@pytest.mark.parametrize('depth', [4, 5])
def test_solve_residual_in_the_models_system(sphere, model, depth):
    """|b - A chi_dev| / |b| <= 2 cg_tol in float64 with the model's A and b; iterations in 1 .. max_iters; n_occ exactly,
    lambda, lo, h to 1e-6.  chi_dev = volume + iso: the border rule changes nothing on this input (the border lies outside
    the sphere, where chi - iso < 0; were that not so the residual would fail).  iso: the exact value is 0 (the columns of g
    sum to 0, so 1 . b = 0 = lambda n iso), a relative bound on it alone means nothing; the device's iso must equal the
    model's formula mean((W chi_dev)_p) to 1e-6 of the sum over absolute values of that mean's terms.  The residual the
    finest level reports is the recurrence's: <= cg_tol where the level stopped before max_iters, and within cg_tol of the
    true one (the slack that 2 cg_tol above already grants)."""
    from points2surf_amd import poisson
    pts, nrm = sphere
    chi_m, lev = model[depth]
    verts, faces, vol, rep = poisson.reconstruct(pts, nrm, depth=depth, cg_tol=CG_TOL, max_iters=MAX_ITERS, want_volume=True,
                                                 want_report=True)
    vol = vol.cpu().numpy().astype(np.float64)
    assert (vol[P.border_mask(lev.R)] <= 0).all()
    chi = vol.reshape(-1) + rep['iso']
    res = np.linalg.norm(lev.b - lev.A @ chi) / np.linalg.norm(lev.b)
    print('depth', depth, 'residual', res, 'report', rep)
    assert res <= 2.0 * CG_TOL
    _check_reported_residual(rep, res)
    assert len(rep['levels']) == depth - 2
    for lv in rep['levels']:
        m = P.Level(pts, nrm, lv['depth'])
        assert 1 <= lv['iterations'] <= MAX_ITERS and lv['n_occ'] == m.n_occ and abs(lv['lam'] - m.lam) <= 1e-6 * m.lam
    assert abs(rep['h'] - lev.h) <= 1e-6 * lev.h and np.abs(np.array(rep['lo']) - lev.lo).max() <= 1e-6 * np.abs(lev.lo).max()
    iso_formula, iso_scale = P.iso_value(lev, chi), float(np.mean(lev.W @ np.abs(chi)))
    print('iso', rep['iso'], 'formula on chi_dev', iso_formula, 'scale', iso_scale, 'model', P.iso_value(lev, chi_m))
    assert abs(rep['iso'] - iso_formula) <= 1e-6 * iso_scale


def _info(verts, faces):
    from points2surf_amd import gt_sdf
    m = gt_sdf.TriMesh(verts, faces)
    try:
        return m.info()
    finally:
        m.close()


def _model_mesh(lev, chi):
    """the model's volume through the same p2s_marching_cubes, vertices in model space"""
    from points2surf_amd import engine
    vol, _ = P.volume(lev, chi)
    v, f, _ = engine.marching_cubes(torch.from_numpy(vol).cuda(), model_space=False, fix_inversion=True)
    return lev.lo + lev.h * v.cpu().numpy().astype(np.float64), f


def test_surface_of_the_sphere(sphere, model):
    """closed, not inverted, Euler characteristic 2, every vertex within 0.5 h of the sphere, as many components as the
    model's volume gives"""
    from points2surf_amd import poisson
    chi_m, lev = model[5]
    verts, faces = poisson.reconstruct(sphere[0], sphere[1], depth=5, cg_tol=CG_TOL, max_iters=MAX_ITERS)
    info = _info(verts, faces)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    edges = np.sort(faces.cpu().numpy()[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    E = np.unique(edges, axis=0).shape[0]
    err = np.abs(np.linalg.norm(verts.cpu().numpy().astype(np.float64), axis=1) - 0.5) / lev.h
    vm, fm = _model_mesh(lev, chi_m)
    info_m = _info(torch.from_numpy(vm.astype(np.float32)), fm)
    print('V', V, 'F', F, 'E', E, info, 'max error / h', err.max(), 'model', info_m, np.abs(np.linalg.norm(vm, axis=1) - 0.5).max() / lev.h)
    assert info['closed'] and not info['inverted'] and V - E + F == 2
    assert err.max() <= 0.5
    assert info['components'] == info_m['components']


def _euler(verts, faces):
    edges = np.sort(faces.cpu().numpy()[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    return int(verts.shape[0]) - np.unique(edges, axis=0).shape[0] + int(faces.shape[0])


def test_solve_at_depth_7():
    """R = 129, 40000 points, levels 3 .. 7.  R^3 / 1024 = 2097 workgroups wanted by the CG's vector kernels, PS_MAX_PART
    launched: ps_cg_* stride and ps_sum_partials adds 1024 partials; p . A p comes from ps_stencil_kernel's tile-strided
    workgroups.  The residual in the matrix-free model's A and b as in test_solve_residual_in_the_models_system, the
    reported residual, n_occ, lambda, lo, h, the iso formula; the surface closed with Euler characteristic 2."""
    from points2surf_amd import poisson
    pts, nrm, _ = MORE['sphere40k']
    lev = _free('sphere40k', 7)
    shape = _launch(lev, 40000)
    assert shape['g_vec_wanted'] > PS_MAX_PART and shape['n_tiles'] > PS_MAX_PART
    verts, faces, vol, rep = poisson.reconstruct(pts, nrm, depth=7, cg_tol=CG_TOL, max_iters=MAX_ITERS, want_volume=True,
                                                 want_report=True)
    vol = vol.cpu().numpy().astype(np.float64)
    assert (vol[P.border_mask(lev.R)] <= 0).all()
    chi = vol.reshape(-1) + rep['iso']
    res = np.linalg.norm(lev.b - lev.apply(chi)) / np.linalg.norm(lev.b)
    print('depth 7 residual', res, 'report', rep)
    assert res <= 2.0 * CG_TOL
    _check_reported_residual(rep, res)
    assert len(rep['levels']) == 5
    for lv in rep['levels']:
        m = _free('sphere40k', lv['depth'])
        assert 1 <= lv['iterations'] <= MAX_ITERS and lv['n_occ'] == m.n_occ and abs(lv['lam'] - m.lam) <= 1e-6 * m.lam
    assert abs(rep['h'] - lev.h) <= 1e-6 * lev.h and np.abs(np.array(rep['lo']) - lev.lo).max() <= 1e-6 * np.abs(lev.lo).max()
    iso_formula, iso_scale = P.iso_value(lev, chi), float(np.mean(lev.W @ np.abs(chi)))
    print('iso', rep['iso'], 'formula on chi_dev', iso_formula, 'scale', iso_scale)
    assert abs(rep['iso'] - iso_formula) <= 1e-6 * iso_scale
    info = _info(verts, faces)
    print('V', verts.shape[0], 'F', faces.shape[0], info)
    assert info['closed'] and not info['inverted'] and _euler(verts, faces) == 2


ONE_STEP_MARGIN = 4.0


@pytest.mark.parametrize('depth', [5, 7])
def test_one_cg_step_per_level_is_the_models_cascade(sphere, depth):
    """cg_tol = 1e30 stops every level after its first iteration, so the volume is the cascade of prolongation and one
    Jacobi-preconditioned CG step per level, 3 .. depth: ps_prolong_kernel's weights, alpha, the update of x.  Compared at
    every node with the float64 one_step_cascade (on the border, where the volume holds -|chi - iso|, by absolute value).
    The tolerance is measured, not chosen: d32 = the distance of the model's float32-store emulation from its float64
    cascade; the device, which also sums in another order, must lie within 4 d32.  A prolongation with half the weight on
    the odd nodes lies a million times further away (tests/test_poisson_model.py).
    Depth 5: the 20000-point sphere.  Depth 7: the 40000-point one; there alpha's p . A p is the sum that
    ps_stencil_kernel's workgroups carry over their strided tiles and that ps_sum_partials adds from PS_MAX_PART partials,
    and a wrong alpha shows here at once, while a full solve only takes more iterations over it."""
    from points2surf_amd import poisson
    pts, nrm = sphere if depth == 5 else MORE['sphere40k'][:2]
    c64, lev = P.one_step_cascade(pts, nrm, depth)
    c32, _ = P.one_step_cascade(pts, nrm, depth, np.float32)
    if depth == 7:
        shape = _launch(lev, pts.shape[0])
        assert shape['n_tiles'] > PS_MAX_PART and shape['g_vec_wanted'] > PS_MAX_PART
    _, _, vol, rep = poisson.reconstruct(pts, nrm, depth=depth, cg_tol=1e30, max_iters=8, want_volume=True, want_report=True)
    assert [lv['iterations'] for lv in rep['levels']] == [1] * (depth - 2)
    vol = vol.cpu().numpy().astype(np.float64).reshape(-1)
    border = P.border_mask(lev.R).reshape(-1)
    assert (~border).sum() == (lev.R - 2) ** 3
    diff = np.where(border, np.abs(vol) - np.abs(c64 - rep['iso']), vol + rep['iso'] - c64)
    d32, d_dev = np.abs(c32 - c64).max(), np.abs(diff).max()
    print('depth', depth, 'max |chi|', np.abs(c64).max(), 'd32', d32, 'device', d_dev, 'device / d32', d_dev / d32)
    assert np.abs(c64).max() > 0 and d32 > 0
    assert d_dev <= ONE_STEP_MARGIN * d32


def test_levels_that_stop_unconverged(sphere):
    """max_iters = 3 is no multiple of PS_CHECK_EVERY and cg_tol = 1e-12 is out of float32's reach: every level makes 3
    iterations and says so, the mesh call still answers with counts, and two calls give the same bytes"""
    from points2surf_amd import poisson
    assert 3 % PS_CHECK_EVERY != 0
    pts, nrm = sphere
    a = poisson.reconstruct(pts, nrm, depth=4, cg_tol=1e-12, max_iters=3, want_volume=True, want_report=True)
    b = poisson.reconstruct(pts, nrm, depth=4, cg_tol=1e-12, max_iters=3, want_volume=True, want_report=True)
    print(a[3])
    for rep in (a[3], b[3]):
        assert [lv['iterations'] for lv in rep['levels']] == [3, 3]
        assert all(lv['residual'] > 1e-12 for lv in rep['levels'])
    for x, y in zip(a[:3], b[:3]):
        assert x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert np.isfinite(a[2].cpu().numpy()).all()
    rc, _, _, _, nv, nf = _raw_call(pts, nrm, depth=4, max_iters=3, cg_tol=1e-12)
    assert rc in (0, -4) and nv > 0 and nf > 0                                  # P2S_OK or P2S_ECAPACITY, with the counts
    assert (nv, nf) == (a[0].shape[0], a[1].shape[0])


def test_iso_of_more_points_than_one_pass():
    """263000 points at depth 3: ps_iso_kernel wants 1028 workgroups, PS_MAX_PART are launched and stride; the device's iso
    against the model's formula on the device's own chi"""
    from points2surf_amd import poisson
    pts, nrm, scale = MORE['many_points']
    lev = _free('many_points', 3)
    assert _launch(lev, pts.shape[0])['g_points_wanted'] > PS_MAX_PART
    _, _, vol, rep = poisson.reconstruct(pts, nrm, depth=3, scale=scale, want_volume=True, want_report=True)
    vol = vol.cpu().numpy().astype(np.float64).reshape(-1)
    border = P.border_mask(lev.R).reshape(-1)
    # the volume holds -|chi - iso| on the border; the sphere's cells end two nodes short of it and only the two corner
    # points, 2 of 263000, reach it, outside the sphere where chi - iso < 0: were that not so the formula would not hold
    assert (vol[border] <= 0).all()
    chi = vol + rep['iso']
    iso_formula, iso_scale = float(np.mean(lev.W64 @ chi)), float(np.mean(lev.W64 @ np.abs(chi)))
    print('iso', rep['iso'], 'formula on chi_dev', iso_formula, 'scale', iso_scale, 'border nodes in reach of a point',
          int(np.intersect1d(np.unique(lev.W64.indices), np.nonzero(border)[0]).size))
    assert abs(rep['iso'] - iso_formula) <= 1e-6 * iso_scale


UZ_CUT, UZ_LIMIT = 0.6, 0.5       # points with u_z >= UZ_CUT removed; vertices with u_z < UZ_LIMIT are held to the bound


def test_open_scan_is_closed_by_the_border_rule(sphere):
    """the sphere without its cap, depth 5: the mesh is closed, no border node is positive, the vertices away from the hole
    (u_z < 0.5) lie within 0.5 h of the sphere -- on the model's own mesh too, which is what fixes the limit 0.5"""
    from points2surf_amd import poisson
    keep = sphere[1][:, 2] < UZ_CUT
    pts, nrm = sphere[0][keep], sphere[1][keep]
    verts, faces, vol, rep = poisson.reconstruct(pts, nrm, depth=5, cg_tol=CG_TOL, max_iters=MAX_ITERS, want_volume=True, want_report=True)
    chi_m, lev, _ = P.solve(pts, nrm, 5)
    vm, _ = _model_mesh(lev, chi_m)

    def worst(v):
        v = np.asarray(v, np.float64)
        r = np.linalg.norm(v, axis=1)
        sel = v[:, 2] / r < UZ_LIMIT
        return np.abs(r[sel] - 0.5).max() / lev.h, int(sel.sum())
    w_dev, w_model = worst(verts.cpu().numpy()), worst(vm)
    info = _info(verts, faces)
    print('device', w_dev, 'model', w_model, info)
    assert w_model[0] <= 0.5 and w_model[1] > 0
    assert info['closed'] and (vol.cpu().numpy()[P.border_mask(lev.R)] <= 0).all()
    assert w_dev[0] <= 0.5 and w_dev[1] > 0


def test_two_calls_give_the_same_bytes(sphere):
    from points2surf_amd import poisson
    a = poisson.reconstruct(sphere[0], sphere[1], depth=5, want_volume=True)
    b = poisson.reconstruct(sphere[0], sphere[1], depth=5, want_volume=True)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert a[0].shape[0] > 0 and a[1].shape[0] > 0


def _raw_call(pts, nrm, depth=4, point_weight=4.0, scale=1.1, cap_v=64, cap_f=64, n=None, max_iters=100, cg_tol=1e-3):
    """p2s_poisson_reconstruct with sentinel-filled outputs: (rc, volume, verts, faces, n_verts, n_faces)"""
    from points2surf_amd import _lib, engine, poisson
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
    q = torch.from_numpy(np.ascontiguousarray(nrm, np.float32)).to(dev)
    R = 2 ** min(max(depth, 3), 9) + 1
    vol = torch.full((R, R, R), 7.0, dtype=torch.float32, device=dev)
    verts = torch.full((max(cap_v, 1), 3), 7.0, dtype=torch.float32, device=dev)
    faces = torch.full((max(cap_f, 1), 3), 7, dtype=torch.int32, device=dev)
    prm = poisson.Params(depth, max_iters, point_weight, scale, cg_tol)
    nv, nf = ctypes.c_int64(-7), ctypes.c_int64(-7)
    info = (ctypes.c_double * poisson.INFO)()
    rc = lib.p2s_poisson_reconstruct(engine._ptr(p), engine._ptr(q), p.shape[0] if n is None else n, ctypes.byref(prm), engine._ptr(vol),
                                     engine._ptr(verts), cap_v, engine._ptr(faces), cap_f, ctypes.byref(nv), ctypes.byref(nf), info,
                                     dev.index, engine._stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, vol, verts, faces, nv.value, nf.value


def _refusals():
    pts, nrm = P.sphere(500, 9)
    bad_p, bad_n = pts.copy(), nrm.copy()
    bad_p[17, 1] = np.nan
    bad_n[499, 2] = np.inf
    return {
        'no_points': dict(pts=pts, nrm=nrm, n=0),
        'non_finite_point': dict(pts=bad_p, nrm=nrm),
        'non_finite_normal': dict(pts=pts, nrm=bad_n),
        'all_normals_zero': dict(pts=pts, nrm=np.zeros_like(nrm)),
        'no_extent': dict(pts=np.repeat(pts[:1], 50, 0), nrm=nrm[:50]),
        'point_weight_zero': dict(pts=pts, nrm=nrm, point_weight=0.0),
        'scale_below_one': dict(pts=pts, nrm=nrm, scale=0.99),
        'depth_2': dict(pts=pts, nrm=nrm, depth=2),
        'depth_10': dict(pts=pts, nrm=nrm, depth=10),
    }


REFUSALS = _refusals()


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refusals_write_nothing(case):
    rc, vol, verts, faces, nv, nf = _raw_call(**REFUSALS[case])
    assert rc == -1                                                            # P2S_EINVAL
    assert (vol == 7.0).all() and (verts == 7.0).all() and (faces == 7).all() and nv == -7 and nf == -7


def test_capacity_zero_reports_the_counts_and_a_second_call_succeeds():
    pts, nrm = P.sphere(2000, 3)
    rc, _, verts, faces, nv, nf = _raw_call(pts, nrm, cap_v=0, cap_f=0)
    assert rc == -4 and nv > 0 and nf > 0                                      # P2S_ECAPACITY
    assert (verts == 7.0).all() and (faces == 7).all()
    rc, _, verts, faces, nv2, nf2 = _raw_call(pts, nrm, cap_v=nv, cap_f=nf)
    assert rc == 0 and (nv2, nf2) == (nv, nf)
    f = faces.cpu().numpy()
    assert f.min() == 0 and f.max() == nv - 1 and np.isfinite(verts.cpu().numpy()).all()
    rc, _, _, _, nv3, nf3 = _raw_call(pts, nrm, cap_v=nv - 1, cap_f=nf)
    assert rc == -4 and (nv3, nf3) == (nv, nf)
