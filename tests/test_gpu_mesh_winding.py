"""Hierarchical winding number on the device (p2s_mesh_winding, p2s_mesh_distance signed_ 2; p2s_md_wtree_kernel) against
the exact sum on the same handle (p2s_md_winding_kernel), on the fixture meshes, on an opened mesh and at the edges."""
import os
import shutil

import numpy as np
import pytest

from test_mesh_sdf_model import GOLDEN, MESHES, load

pytestmark = pytest.mark.gpu
TAU = 2.0 ** -10
OPENED = '00016513'


def _np(t):
    return t.cpu().numpy()


def _tree(mesh, q, tau=TAU):
    w, e, st = mesh.winding(q, method='tree', tau=tau, want_bound=True, want_stats=True)
    return _np(w), _np(e), st


def _opened(v, f):
    cz = v.astype(np.float64)[f].mean(1)[:, 2]
    keep = cz < np.quantile(cz, 0.95)
    assert (~keep).sum() == 266
    return f[keep]


@pytest.fixture(scope='module')
def cases():
    from points2surf_amd import gt_sdf
    out = {}
    for name in MESHES:
        v, f, q, _ = load(name)
        q = q.astype(np.float32)
        mesh = gt_sdf.TriMesh(v, f)
        out[name] = dict(v=v, f=f, q=q, mesh=mesh, exact=_np(mesh.winding(q, method='exhaustive')))
    yield out
    for c in out.values():
        c['mesh'].close()


def _check(mesh, q, exact, tau):
    """the contract of the tree: |w~ - w_exact| <= eps, eps <= tau + rounding term, same decision; returns the stats"""
    from points2surf_amd import gt_sdf
    info = mesh.info()
    w, e, st = _tree(mesh, q, tau)
    diff = np.abs(w - exact)
    print('faces', info['n_faces'], 'tau', tau, 'max |w~ - w|', diff.max(), 'max eps', e.max(), st)
    assert (diff <= e).all()
    assert (e <= tau + gt_sdf.winding_rounding(info['n_faces'], info['n_faces'], info['degenerate'])).all()
    assert ((np.abs(w) > 0.5) == (np.abs(exact) > 0.5)).all()
    assert st['triangles'] + st['accepted'] <= len(q) * info['n_faces']
    return w, e, st


def test_tree_against_the_exact_sum_on_the_fixtures(cases):
    for name, c in cases.items():
        assert np.abs(c['exact'] - np.round(c['exact'])).max() < 1e-9          # closed: an integer
        _, _, st = _check(c['mesh'], c['q'], c['exact'], TAU)
        assert st['redecided'] == 0
        # where the budget rule accepts nodes: the largest tau, and queries up to four box sizes away
        far = np.random.RandomState(len(c['f'])).uniform(-4, 4, (2000, 3)).astype(np.float32)
        far_exact = _np(c['mesh'].winding(far, method='exhaustive'))
        accepted = 0
        for q, ex in ((c['q'], c['exact']), (far, far_exact)):
            for tau in (TAU, 0.25):
                accepted += _check(c['mesh'], q, ex, tau)[2]['accepted']
        assert accepted > 0


def test_distance_signed_by_winding_equals_the_pseudonormal_sign(cases):
    for name, c in cases.items():
        a = _np(c['mesh'].distance(c['q'], signed=True))
        b, fb = c['mesh'].distance(c['q'], signed='winding', want_face=True)
        assert np.array_equal(a, _np(b)), name
        assert c['mesh'].n_winding == 0
        e = _np(c['mesh'].distance(c['q'], signed='winding', method='exhaustive'))
        assert np.array_equal(a, e)
    with pytest.raises(ValueError):
        c['mesh'].distance(c['q'], signed='sideways')


def test_opened_mesh(cases):
    """00016513 without the 266 faces whose centroid z is at or above the 0.95-quantile.  On the CPU the exact sum puts no
    fixture query within 1e-3 of 0.5 (the minimum is 2.06e-3), so at tau = 2^-10 the tree decides (nearly) all of them: at
    most 1 % may be re-decided."""
    from points2surf_amd import _lib, gt_sdf
    c = cases[[n for n in MESHES if n.startswith(OPENED)][0]]
    mesh = gt_sdf.TriMesh(c['v'], _opened(c['v'], c['f']))
    q = c['q']
    assert not mesh.info()['closed']
    with pytest.raises(_lib.P2SError) as ei:
        mesh.distance(q, signed=True)
    assert ei.value.code == -1
    unsigned = _np(mesh.distance(q, signed=False))
    d = _np(mesh.distance(q, signed='winding'))
    redecided = mesh.n_winding
    exact = _np(mesh.winding(q, method='exhaustive'))
    print('min | |w| - 0.5 |', np.abs(np.abs(exact) - 0.5).min(), 're-decided', redecided)
    assert np.array_equal(np.abs(d), unsigned)
    far = unsigned > 1e-8
    assert ((d > 0) == (np.abs(exact) > 0.5))[far].all() and (d[~far] == unsigned[~far]).all()
    assert redecided <= 0.01 * len(q)
    w, e, st = _check(mesh, q, exact, TAU)
    assert st['redecided'] == redecided
    assert (np.abs(exact) > 0.5).any() and (np.abs(exact) < 0.5).any()
    mesh.close()


TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]]))
TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]))


@pytest.mark.parametrize('shape', ['triangle', 'tetrahedron'])
def test_edges(shape):
    from points2surf_amd import gt_sdf
    v, f = TRIANGLE if shape == 'triangle' else TETRA
    mesh = gt_sdf.TriMesh(v, f)
    lo, hi = v.min(0), v.max(0)
    special = np.array([v[0], v[1], 0.5 * (v[0] + v[1]), [0.25, 0.25, 0.0], 0.5 * (lo + hi)], np.float32)   # vertex, edge, in a face, box centre
    rnd = np.random.RandomState(5).uniform(-1.5, 2.5, (60, 3)).astype(np.float32)
    q = np.concatenate([special, rnd])
    assert len(q) == 65                                              # a partial wave
    exact = _np(mesh.winding(q, method='exhaustive'))
    assert np.isfinite(exact).all()
    if shape == 'triangle':
        assert abs(exact[3]) == 0.5                                  # in the plane of the face, inside it
    for tau in (TAU, 0.25):
        w, e, st = _check(mesh, q, exact, tau)
        undecided = (e == 0)                                         # re-decided: the exact value, bound 0
        assert np.isfinite(w).all() and st['redecided'] == undecided.sum()
        assert np.array_equal(w[undecided], exact[undecided])
        assert (np.abs(np.abs(w[~undecided]) - 0.5) > e[~undecided]).all()
        assert undecided[3] or shape != 'triangle'
    # far away: the root is taken as one dipole.  The triangle is seen from a point of its own plane (w = 0 exactly; from
    # anywhere else its true w is A cos / (4 pi d^2) > eps), the closed tetrahedron from any direction (N = 0)
    far = np.array([[1e6, 0, 0], [0, -1e6, 0], [6e5, 8e5, 0]] + ([] if shape == 'triangle' else [[0, 0, 1e6], [-6e5, 0, 8e5]]), np.float32)
    w, e, st = _tree(mesh, far)
    assert (np.abs(w) <= e).all() and st['accepted'] == len(far) and st['triangles'] == 0 and st['redecided'] == 0
    assert (e <= gt_sdf.winding_rounding(len(f), 1) + 1e-15).all()
    # non-finite queries
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.2, 0.2, 0.2], [0, 0, -np.inf]], np.float32)
    for method in ('tree', 'exhaustive'):
        w, e = mesh.winding(bad, method=method, want_bound=True)
        w, e = _np(w), _np(e)
        assert np.isnan(w[[0, 1, 3]]).all() and np.isnan(e[[0, 1, 3]]).all() and np.isfinite(w[2]) and np.isfinite(e[2])
    assert np.isnan(_np(mesh.distance(bad, signed='winding'))[[0, 1, 3]]).all()
    # n = 0
    w, e, st = mesh.winding(np.zeros((0, 3), np.float32), want_bound=True, want_stats=True)
    assert w.shape[0] == 0 and e.shape[0] == 0 and st == dict(accepted=0, triangles=0, redecided=0)
    assert mesh.distance(np.zeros((0, 3), np.float32), signed='winding').shape[0] == 0
    # tau = 0 opens everything
    w, e, st = _tree(mesh, q, 0.0)
    assert st['accepted'] == 0 and np.abs(w - exact).max() <= 1e-12 and (np.abs(w - exact) <= e).all()
    mesh.close()


def test_zero_area_face(cases):
    from points2surf_amd import gt_sdf
    v, f = TETRA
    f2 = np.concatenate([f, [[0, 1, 1]]])
    mesh = gt_sdf.TriMesh(v, f2)
    assert mesh.info()['degenerate'] == 1
    q = np.concatenate([np.random.RandomState(11).uniform(-2, 3, (200, 3)), [[0.5, 0, 0], [0.1, 0.1, 0.1], [1e6, 0, 0]]]).astype(np.float32)
    exact = _np(mesh.winding(q, method='exhaustive'))
    assert np.isfinite(exact).all()
    for tau in (TAU, 0.25, 0.0):
        w, e, st = _check(mesh, q, exact, tau)
        assert np.isfinite(w).all()
    mesh.close()


def test_tau_out_of_range_is_refused(cases):
    import torch
    from points2surf_amd import _lib
    c = cases[MESHES[0]]
    for tau in (-1e-9, float('nan'), 0.3, float('inf')):
        for method in ('tree', 'exhaustive'):
            with pytest.raises(_lib.P2SError) as ei:
                c['mesh'].winding(c['q'][:8], method=method, tau=tau)
            assert ei.value.code == -1
    # nothing written: straight through the C ABI on a pre-filled buffer
    import ctypes
    from points2surf_amd import engine
    q = torch.from_numpy(c['q'][:8]).cuda()
    w = torch.full((8,), 7.0, dtype=torch.float64, device='cuda')
    st = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    rc = c['mesh'].lib.p2s_mesh_winding(c['mesh'].handle, engine._ptr(q), 8, 0, 0.3, engine._ptr(w), None, st, engine._stream_ptr(q.device))
    torch.cuda.synchronize()
    assert rc == -1 and (_np(w) == 7.0).all() and list(st) == [0, 0, 0, 0]
    rc = c['mesh'].lib.p2s_mesh_winding(c['mesh'].handle, engine._ptr(q), 8, 2, TAU, engine._ptr(w), None, st, engine._stream_ptr(q.device))
    assert rc == -1 and (_np(w) == 7.0).all()


def test_more_than_16_components():
    """17 disjoint tetrahedra: signed=True takes the all-winding path (exact sum per query), 'winding' the tree"""
    from points2surf_amd import gt_sdf
    v0, f0 = TETRA
    v = np.concatenate([v0 * 0.5 + np.array([1.5 * (k % 5), 1.5 * (k // 5), 0.25 * k], np.float32) for k in range(17)])
    f = np.concatenate([f0 + 4 * k for k in range(17)])
    assert len(f) == 68
    mesh = gt_sdf.TriMesh(v, f)
    assert mesh.info()['closed'] and mesh.info()['components'] == 17
    rs = np.random.RandomState(17)
    inside = np.concatenate([(v0 * 0.5).mean(0) + np.array([1.5 * (k % 5), 1.5 * (k // 5), 0.25 * k]) + rs.uniform(-0.03, 0.03, (20, 3)) for k in range(17)])
    q = np.concatenate([rs.uniform(-1, 7, (1000, 3)), inside]).astype(np.float32)
    a = _np(mesh.distance(q, signed=True))
    assert mesh.n_winding > 0
    b = _np(mesh.distance(q, signed='winding'))
    assert np.array_equal(a, b) and (a[1000:] > 0).all() and (a < 0).any()
    mesh.close()


def test_reproducible(cases):
    from points2surf_amd import gt_sdf
    c = cases[MESHES[0]]
    far = np.random.RandomState(3).uniform(-4, 4, (2000, 3)).astype(np.float32)
    q = np.concatenate([c['q'], far])
    other = gt_sdf.TriMesh(c['v'], c['f'])
    for tau in (TAU, 0.25):
        w0, e0, s0 = _tree(c['mesh'], q, tau)
        w1, e1, s1 = _tree(c['mesh'], q, tau)
        w2, e2, s2 = _tree(other, q, tau)
        assert np.array_equal(w0, w1) and np.array_equal(e0, e1) and s0 == s1
        assert np.array_equal(w0, w2) and np.array_equal(e0, e2) and s0 == s2
    other.close()


def test_gt_sdf_sign_winding_and_sdf_error(cases, tmp_path):
    from points2surf_amd import gt_sdf, metrics, ply
    name = [n for n in MESHES if n.startswith(OPENED)][0]
    c = cases[name]
    data = tmp_path / 'open_set'
    (data / '03_meshes').mkdir(parents=True)
    (data / '05_query_pts').mkdir()
    ply.write_ply(str(data / '03_meshes' / name), c['v'], _opened(c['v'], c['f']))
    shutil.copy(os.path.join(GOLDEN, '05_query_pts', name + '.npy'), str(data / '05_query_pts' / (name + '.npy')))
    with pytest.raises(ValueError, match='is not closed'):
        gt_sdf.main(['--indir', str(data)])
    assert not os.path.exists(str(data / '05_query_dist' / (name + '.npy')))
    gt_sdf.main(['--indir', str(data), '--sign', 'winding'])
    d = np.load(str(data / '05_query_dist' / (name + '.npy')))
    assert d.dtype == np.float32 and d.shape == (2000,) and np.isfinite(d).all() and np.abs(d).max() <= 1.0
    assert (d > 0).any() and (d < 0).any()
    rec = tmp_path / 'rec'
    (rec / 'dist_ms').mkdir(parents=True)
    (rec / 'query_pts_ms').mkdir()
    stem = name[:-4] + '.xyz.npy'
    np.save(str(rec / 'dist_ms' / stem), d)
    np.save(str(rec / 'query_pts_ms' / stem), c['q'])
    rows = metrics.sdf_error(str(rec), str(data / '03_meshes'), str(tmp_path / 'a.csv'))
    assert rows[0][-1] == '-1'
    rows = metrics.sdf_error(str(rec), str(data / '03_meshes'), str(tmp_path / 'b.csv'), sign='winding')
    assert len(rows) == 1 and rows[0][-1] != '-1' and float(rows[0][-1]) == 0.0 and int(rows[0][2]) == 2000
    assert float(rows[0][5]) <= 1e-7                                      # the file is the float32 rounding of the same distances
    assert open(str(tmp_path / 'b.csv')).read().split('\n')[1].split(',')[-1] != '-1'
