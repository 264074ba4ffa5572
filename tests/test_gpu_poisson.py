"""The Screened Poisson baseline on the device (points2surf_amd.poisson: p2s_poisson_system, p2s_poisson_reconstruct)
against its float64 model (tests/poisson_model.py): the pieces of one level node by node within a rounding bound, the
solve by its residual in the model's A and b, the surface, an open scan, determinism, refusals and capacities."""
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


def _sphere(n, seed):
    return P.sphere(n, seed)


def _cases():
    rng = np.random.default_rng(5)
    unit = np.array([[0.0, 0.6, 0.8]], np.float32)
    corners = np.array([[0, 0, 0], [1, 1, 1]], np.float32)
    out = {}
    # one point inside a cell; two points without normals span the box
    out['inside'] = (np.concatenate([np.array([[0.30, 0.41, 0.52]], np.float32), corners]),
                     np.concatenate([unit, np.zeros((2, 3), np.float32)]), 1.1)
    # one point exactly on a node of both depths; scale 1.0 puts the corner points on the last node (the clamp, t = 1)
    out['on_node_scale1'] = (np.concatenate([np.array([[0.5, 0.25, 0.75]], np.float32), corners]),
                             np.concatenate([unit, np.array([[1, 0, 0], [0, -2, 0.5]], np.float32)]), 1.0)
    # 300 identical points in one cell and 5 elsewhere: the ends of the cell sort's segments
    few = rng.random((5, 3)).astype(np.float32)
    out['dense_cell'] = (np.concatenate([np.repeat(np.array([[0.61, 0.33, 0.47]], np.float32), 300, 0), few, corners]),
                         np.concatenate([np.repeat(unit, 300, 0), rng.standard_normal((5, 3)).astype(np.float32),
                                         np.zeros((2, 3), np.float32)]), 1.1)
    out['sphere'] = _sphere(2000, 3) + (1.1,)
    # normals of length 0 for half of the points; scale 1.0: the extreme points of a real cloud on the last node
    pts, nrm = _sphere(2000, 4)
    nrm = nrm.copy()
    nrm[::2] = 0.0
    out['half_zero_scale1'] = (pts, nrm, 1.0)
    return out


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


@pytest.mark.parametrize('depth', [4, 5])
def test_solve_residual_in_the_models_system(sphere, model, depth):
    """|b - A chi_dev| / |b| <= 2 cg_tol in float64 with the model's A and b; iterations in 1 .. max_iters; n_occ exactly,
    lambda, lo, h to 1e-6.  chi_dev = volume + iso: the border rule changes nothing on this input (the border lies outside
    the sphere, where chi - iso < 0; were that not so the residual would fail).  iso: the exact value is 0 (the columns of g
    sum to 0, so 1 . b = 0 = lambda n iso), a relative bound on it alone means nothing; the device's iso must equal the
    model's formula mean((W chi_dev)_p) to 1e-6 of the sum over absolute values of that mean's terms."""
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


UZ_CUT, UZ_LIMIT = 0.6, 0.5        # points with u_z >= UZ_CUT removed; vertices with u_z < UZ_LIMIT are held to the bound


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


def _raw_call(pts, nrm, depth=4, point_weight=4.0, scale=1.1, cap_v=64, cap_f=64, n=None):
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
    prm = poisson.Params(depth, 100, point_weight, scale, 1e-3)
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
