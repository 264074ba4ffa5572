"""Normals from the cloud alone on the device (points2surf_amd.normals: p2s_normals_estimate, p2s_normals_orient) against
the float64 model (tests/normals_model.py).

Estimate is checked without relying on the eigen gap.  With C the model's covariance of the (bit-exact) neighbourhood, n
the float32 output and rho its Rayleigh quotient:
    |C n - rho n| <= 2^-22 |C|_F     float32 rounding of a unit vector: |e| <= sqrt(3) 2^-25, residual <= 2 |C| |e| ~ 1e-7 |C|
    rho - lambda_0 <= 2^-44 |C|_F    the excess is second order in e: ~ 5e-15 |C|; a float32 eigen-solver fails this one
    | |n| - 1 | <= 2^-22
(numpy's own eigenvector rounded to float32 reaches 0.17 and 0.03 of the first two).  Orient is exact: the minimum spanning
forest under a total order is unique, so signs, components and counts equal the model's bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import normals_model as M

pytestmark = pytest.mark.gpu

KS = (4, 16)


def _estimate_clouds(k):
    rng = np.random.default_rng(11)
    out = {}
    out['blob'] = (0.2 * rng.standard_normal((1500, 3))).astype(np.float32)
    out['plane'] = np.concatenate([rng.uniform(-0.5, 0.5, (1200, 2)), np.zeros((1200, 1))], axis=1).astype(np.float32)
    # exactly collinear in float32: multiples of 2^-12 along (1, 2, -1)
    t = rng.permutation(4096)[:600].astype(np.float64) * 2.0 ** -12 - 0.5
    out['line'] = np.stack([t, 2.0 * t, -t], axis=1).astype(np.float32)
    out['slab'] = (rng.uniform(-0.5, 0.5, (2000, 3)) * np.array([1.0, 1.0, 1e-3])).astype(np.float32)
    base = rng.uniform(-0.5, 0.5, (700, 3)).astype(np.float32)
    out['duplicated'] = np.concatenate([base, base])
    out['coincident'] = np.concatenate([np.repeat(np.array([[0.1, -0.2, 0.3]], np.float32), k, 0),
                                        rng.uniform(-0.5, 0.5, (1000, 3)).astype(np.float32)])
    return out


CLOUD_NAMES = ('blob', 'plane', 'line', 'slab', 'duplicated', 'coincident')


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', CLOUD_NAMES)
def test_estimate_residual_rayleigh_and_length(name, k):
    from points2surf_amd import engine, normals
    pts = _estimate_clouds(k)[name]
    _, var_m, C, lam, ids = M.estimate(pts, k)
    cloud = engine.Cloud(pts)
    try:
        got_ids = cloud.knn_patch(cloud.pts, k, want_patch=False)[0].cpu().numpy()
        nrm, var = normals.estimate(cloud, k=k, orient='none')
    finally:
        cloud.close()
    assert np.array_equal(got_ids, ids)
    assert nrm.dtype == torch.float32 and tuple(nrm.shape) == (len(pts), 3) and tuple(var.shape) == (len(pts),)
    n32, var = nrm.cpu().numpy(), var.cpu().numpy()
    n = n32.astype(np.float64)
    fro = np.sqrt((C * C).sum(axis=(1, 2)))
    zero = fro == 0.0
    assert (n32[zero] == 0.0).all() and (var[zero] == 0.0).all()
    if name == 'coincident':
        assert zero[:k].all() and not zero[k:].any()
    else:
        assert not zero.any()
    nz = ~zero
    length = np.linalg.norm(n[nz], axis=1)
    Cn = np.einsum('nij,nj->ni', C[nz], n[nz])
    rho = (n[nz] * Cn).sum(axis=1) / (length * length)
    resid = np.linalg.norm(Cn - rho[:, None] * n[nz], axis=1)
    excess = rho - lam[nz, 0]
    print(name, 'k', k, 'residual / |C|', float((resid / fro[nz]).max()), 'of', 2.0 ** -22, 'excess / |C|', float((excess / fro[nz]).max()),
          'of', 2.0 ** -44, '| |n| - 1 |', float(np.abs(length - 1.0).max()), 'variation', float(np.abs(var - var_m).max()))
    assert (resid <= 2.0 ** -22 * fro[nz]).all()
    assert (excess <= 2.0 ** -44 * fro[nz]).all()
    assert (np.abs(length - 1.0) <= 2.0 ** -22).all()
    assert (np.abs(var.astype(np.float64) - var_m) <= 2.0 ** -22).all()
    if name == 'plane':
        assert (n32[:, :2] == 0.0).all() and (np.abs(n32[:, 2]) == 1.0).all()


# ---- orient ------------------------------------------------------------------------------------------------------------

ANALYTIC = {'sphere': (M.sphere, 8), 'torus': (M.torus, 16), 'two_spheres': (M.two_spheres, 12)}


def _axis_normals(rng, n):
    """normals with exact zeros: +-e_x, +-e_y, +-e_z (pairs exactly orthogonal, d = 0) and zero vectors"""
    nrm = np.zeros((n, 3), np.float32)
    pick = rng.integers(0, 4, n)                         # 3: a zero vector
    for a in range(3):
        nrm[pick == a, a] = rng.choice([-1.0, 1.0], int((pick == a).sum()))
    return nrm


def _orient_inputs(name):
    """(points, normals or None for the device's own estimate, k)"""
    rng = np.random.default_rng(23)
    if name in ANALYTIC:
        make, k = ANALYTIC[name]
        return make()[0], None, k
    if name == 'grid':
        g = np.stack(np.meshgrid(np.arange(40.0), np.arange(40.0), indexing='ij'), -1).reshape(-1, 2) / 64.0 - 0.25
        nrm = np.zeros((1600, 3), np.float32)
        nrm[:, 2] = rng.choice([-1.0, 1.0], 1600)
        return np.concatenate([g, np.zeros((1600, 1))], axis=1).astype(np.float32), nrm, 8
    if name == 'random':
        return rng.uniform(-0.5, 0.5, (3000, 3)).astype(np.float32), M._unit(rng, 3000).astype(np.float32), 6
    if name == 'zeros':
        return rng.uniform(-0.5, 0.5, (1500, 3)).astype(np.float32), _axis_normals(rng, 1500), 10
    if name == 'clusters_k4':
        pts = np.concatenate([0.05 * rng.standard_normal((300, 3)) - 0.4, 0.05 * rng.standard_normal((301, 3)) + 0.4])
        return pts.astype(np.float32), M._unit(rng, 601).astype(np.float32), 4
    if name == 'complete':
        return rng.uniform(-0.5, 0.5, (24, 3)).astype(np.float32), M._unit(rng, 24).astype(np.float32), 24
    raise KeyError(name)


ORIENT_NAMES = ('sphere', 'torus', 'two_spheres', 'grid', 'random', 'zeros', 'clusters_k4', 'complete')


@pytest.mark.parametrize('name', ORIENT_NAMES)
def test_orient_equals_the_model_bit_for_bit(name):
    from points2surf_amd import engine, normals
    pts, nrm, k = _orient_inputs(name)
    cloud = engine.Cloud(pts)
    try:
        if nrm is None:
            nrm = normals.estimate(cloud, k=k, orient='none')[0].cpu().numpy()
        out, rep = normals.orient(cloud, nrm, k=k, want_report=True)
    finally:
        cloud.close()
    out = out.cpu().numpy()
    want, comp, info = M.orient(pts, nrm, k=k)
    print(name, 'k', k, rep['components'], 'components', rep['edges'], 'edges', rep['rounds'], 'rounds', rep['flipped'], 'flipped')
    assert np.array_equal(out.view(np.uint32) & 0x7fffffff, nrm.view(np.uint32) & 0x7fffffff)        # only sign bits change
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(rep['component'].cpu().numpy(), comp)
    assert (rep['components'], rep['edges'], rep['flipped']) == (info['components'], info['edges'], info['flipped'])
    if name == 'grid':
        assert (out == np.array([0.0, 0.0, 1.0], np.float32)).all() and rep['components'] == 1
    if name in ('clusters_k4', 'two_spheres'):
        assert rep['components'] > 1
    if name == 'complete':
        assert rep['edges'] == 24 * 23 // 2 and rep['components'] == 1


@pytest.mark.parametrize('name', sorted(ANALYTIC))
def test_estimate_and_orient_point_outward(name):
    """the clouds on which the model is checked to orient every point (tests/test_normals_model.py)"""
    from points2surf_amd import normals
    pts, truth = ANALYTIC[name][0]()
    nrm, var, rep = normals.estimate(pts, k=12, orient='mst', want_report=True)
    dot = (nrm.cpu().numpy().astype(np.float64) * truth).sum(axis=1)
    print(name, 'components', rep['components'], 'rounds', rep['rounds'], 'wrong', int((dot <= 0).sum()), 'worst |dot|', float(np.abs(dot).min()))
    assert rep['components'] == (2 if name == 'two_spheres' else 1) and rep['k'] == 12
    assert (dot > 0).all()


def test_two_calls_give_equal_bytes():
    from points2surf_amd import normals
    pts = M.torus()[0]
    a = normals.estimate(pts, k=16, orient='mst', want_report=True)
    b = normals.estimate(pts, k=16, orient='mst', want_report=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2]['component'], b[2]['component'])
    assert {x: a[2][x] for x in ('components', 'edges', 'rounds', 'flipped')} == {x: b[2][x] for x in ('components', 'edges', 'rounds', 'flipped')}


def test_refusals():
    from points2surf_amd import _lib, engine, normals
    pts = np.random.default_rng(3).uniform(-0.5, 0.5, (40, 3)).astype(np.float32)
    cloud = engine.Cloud(pts)
    lib = _lib.load()
    s = engine._stream_ptr(cloud.device)
    nrm = torch.zeros((40, 3), dtype=torch.float32, device=cloud.device)
    out = torch.zeros_like(nrm)
    info = (ctypes.c_int64 * 8)()
    try:
        for k in (3, 65, 41):                            # 41 > n = 40
            for call in (lambda: normals.estimate(cloud, k=k), lambda: normals.orient(cloud, nrm, k=k)):
                with pytest.raises(_lib.P2SError) as err:
                    call()
                assert err.value.code == -1
        assert lib.p2s_normals_estimate(cloud.handle, 8, None, None, s) == -1
        assert lib.p2s_normals_estimate(None, 8, engine._ptr(out), None, s) == -1
        assert lib.p2s_normals_orient(cloud.handle, 8, None, engine._ptr(out), None, info, s) == -1
        assert lib.p2s_normals_orient(cloud.handle, 8, engine._ptr(nrm), None, None, info, s) == -1
        bad = nrm.clone()
        bad[7, 1] = float('inf')
        assert lib.p2s_normals_orient(cloud.handle, 8, engine._ptr(bad), engine._ptr(out), None, info, s) == -1
        assert not out.any()                             # nothing was written by a refused call
        # the optional outputs may be NULL
        assert lib.p2s_normals_estimate(cloud.handle, 8, engine._ptr(out), None, s) == 0
        assert lib.p2s_normals_orient(cloud.handle, 8, engine._ptr(out), engine._ptr(out), None, None, s) == 0      # in place
    finally:
        cloud.close()
    with pytest.raises(ValueError):
        normals.estimate(pts, k=8, orient='hoppe')
