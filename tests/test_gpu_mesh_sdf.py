"""Mesh-distance kernels (p2s_trimesh_create, p2s_mesh_distance) on the device against the float64 CPU model
(tests/mesh_sdf_model.py) and the reference's recorded GT data (tests/golden/abc_minimal)."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

import mesh_sdf_model as msm
from test_mesh_sdf_model import GOLDEN, MESHES, load

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALLEST = '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.ply'


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope='module')
def cases():
    from points2surf_amd import gt_sdf
    out = {}
    for name in MESHES:
        v, f, q, g = load(name)
        extra = np.random.RandomState(len(f)).uniform(-1, 1, (2000, 3)).astype(np.float32)
        qa = np.concatenate([q.astype(np.float32), extra])
        m = msm.MeshModel(v, f)
        d, det = m.signed_distance(qa.astype(np.float64), with_details=True)
        out[name] = dict(v=v, f=f, q=qa, g=g, model=m, d=d, det=det, mesh=gt_sdf.TriMesh(v, f))
    yield out
    for c in out.values():
        c['mesh'].close()


def test_exhaustive_kernel_against_the_cpu_model(cases):
    """d^2 within 1e-13 absolute (coordinates below 2, a few dozen float64 operations on either side; the model's two
    formulations, regions vs plane projection, differ by less than 2.5e-14 between themselves --
    test_regions_agree_with_plane_projection -- so the bound stands); same face wherever the model's runner-up is further
    than 1e-12; same sign everywhere"""
    for name, c in cases.items():
        info = c['mesh'].info()
        assert info['closed'] and not info['inverted'] and info['components'] == c['model'].components
        dist, face = c['mesh'].distance(c['q'], signed=True, method='exhaustive', want_face=True)
        dist, face = _np(dist), _np(face)
        err = np.abs(dist * dist - c['det']['d2'])
        print(name[:8], 'max |d2 dev - d2 model|', err.max(), 'winding', c['mesh'].n_winding)
        assert err.max() <= 1e-13
        clear = c['det']['second'] - c['det']['d2'] > 1e-12
        assert (face[clear] == c['det']['face'][clear]).all()
        assert ((dist > 0) == (c['d'] > 0)).all()
        assert c['mesh'].n_winding == int(c['det']['flagged'].sum())


def test_against_the_recorded_distances(cases):
    from points2surf_amd import gt_sdf
    for name, c in cases.items():
        g = c['g'].astype(np.float64)
        dev = _np(c['mesh'].distance(c['q'][:2000], signed=True))
        mod = c['d'][:2000]
        assert (np.abs(np.abs(dev) - np.abs(g)) <= np.abs(np.abs(mod) - np.abs(g)) + 1e-8).all()
        assert ((dev > 0) == (g > 0)).all()
        qd = gt_sdf.query_dist(c['mesh'], c['q'][:2000])
        assert qd.dtype == np.float32
        ulp = np.spacing(np.abs(c['g']))
        model_ok = np.abs(msm.query_dist_post(mod) - c['g']) <= ulp
        assert (np.abs(qd - c['g']) <= ulp)[model_ok].all()


def _both(mesh, q, signed=True):
    a = mesh.distance(q, signed=signed, method='index', want_face=True)
    nw = mesh.n_winding
    b = mesh.distance(q, signed=signed, method='exhaustive', want_face=True)
    assert nw == mesh.n_winding
    return [_np(x) for x in a], [_np(x) for x in b]


def test_index_equals_exhaustive_bit_for_bit(cases, fixture_cloud):
    import torch
    from points2surf_amd import engine
    cloud = engine.Cloud(fixture_cloud)
    grid = cloud.query_grid(128, 3).contiguous()
    assert grid.shape[0] == 68088
    far = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)] +
                   [[s * (a == 0), s * (a == 1), s * (a == 2)] for a in range(3) for s in (-1, 1)], np.float32)
    perm = torch.from_numpy(np.random.RandomState(7).permutation(grid.shape[0])).to(grid.device)
    for name, c in cases.items():
        for q in (grid, far):
            (di, fi), (de, fe) = _both(c['mesh'], q)
            assert np.array_equal(di, de) and np.array_equal(fi, fe), name
        (dp, fp), _ = _both(c['mesh'], grid[perm])
        (di, fi), _ = _both(c['mesh'], grid)
        assert np.array_equal(dp, di[_np(perm)]) and np.array_equal(fp, fi[_np(perm)])
        t = c['mesh'].info()
        print(name[:8], 'faces', t['n_faces'], 'grid', t['grid'])
    c = cases[SMALLEST]
    v, f = c['v'].astype(np.float64), c['f']
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    on = np.concatenate([v, v[e].mean(1), v[f].mean(1)]).astype(np.float32)
    (di, fi), (de, fe) = _both(c['mesh'], on)
    assert np.array_equal(di, de) and np.array_equal(fi, fe)
    assert (di[:len(v)] == 0.0).all()                      # a vertex: exactly 0, unsigned
    assert np.abs(di).max() < 1e-6
    cloud.close()


def test_large_mesh_built_by_the_engine(cases):
    import torch
    from points2surf_amd import _lib, engine, gt_sdf, ply, synth
    pts = np.load(os.path.join(GOLDEN, '04_pts', SMALLEST[:-4] + '.xyz.npy'))
    w, cfg = synth.make_weights('p2s_max')
    model, cloud, rng = engine.Model(w, cfg), engine.Cloud(pts), engine.Rng(40938661)
    sdf, q = engine.infer_shape(model, cloud, rng, 256, 3)
    vol, _ = engine.sdf_volume(q, sdf, 256, 5, 13.0, clamp=True)
    v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
    mv, mf = ply.merge_vertices(v.cpu().numpy(), f.cpu().numpy())
    del vol, v, f, sdf
    mesh = gt_sdf.TriMesh(mv, mf)
    info = mesh.info()
    print('engine mesh', mv.shape, mf.shape, info)
    assert info['n_faces'] == len(mf) > 100000
    qs = cases[SMALLEST]['q'][:2000]
    for signed in ([False, True] if info['closed'] else [False]):
        (di, fi), (de, fe) = _both(mesh, qs, signed=signed)
        assert np.array_equal(di, de) and np.array_equal(fi, fe)
    mesh.distance(qs, signed=False)
    tests = mesh.info()['tests'] / len(qs)
    print('mean triangle tests per query', tests, 'of', len(mf))
    assert tests < len(mf) / 20
    if not info['closed']:
        with pytest.raises(_lib.P2SError) as ei:
            mesh.distance(qs, signed=True)
        assert ei.value.code == -1
    mesh.close()
    cloud.close()


def test_refusals_and_robustness(cases):
    from points2surf_amd import _lib, gt_sdf
    c = cases[SMALLEST]
    v, f, q = c['v'], c['f'], c['q'][:2000]
    want = _np(c['mesh'].distance(q, signed=True))
    # one face removed
    m = gt_sdf.TriMesh(v, f[1:])
    info = m.info()
    assert not info['closed'] and info['bad_edges'] == 3
    with pytest.raises(_lib.P2SError) as ei:
        m.distance(q, signed=True)
    assert ei.value.code == -1
    d2, *_ = msm.nearest(v.astype(np.float64), f[1:], q.astype(np.float64))
    assert np.abs(_np(m.distance(q, signed=False)) ** 2 - d2).max() <= 1e-13
    m.close()
    # every face reversed
    m = gt_sdf.TriMesh(v, f[:, [0, 2, 1]])
    assert m.info()['inverted'] and m.info()['closed']
    assert np.array_equal(_np(m.distance(q, signed=True)), want)
    m.close()
    # bad input
    bad_f = f.copy()
    bad_f[5, 1] = len(v)
    bad_v = v.copy()
    bad_v[3, 2] = np.nan
    for vv, ff in ((v, bad_f), (bad_v, f)):
        with pytest.raises(_lib.P2SError) as ei:
            gt_sdf.TriMesh(vv, ff)
        assert ei.value.code == -1
    # n = 0, F = 1
    assert c['mesh'].distance(np.zeros((0, 3), np.float32)).shape[0] == 0
    m = gt_sdf.TriMesh(np.eye(3, dtype=np.float32), np.array([[0, 1, 2]]))
    assert not m.info()['closed']
    d = _np(m.distance(np.zeros((1, 3), np.float32), signed=False))
    assert abs(d[0] - 1 / np.sqrt(3)) < 1e-15
    m.close()
    # zero-area triangles inside a closed mesh: face (a, b, c) split at a copy M of a into (a, M, c) [zero area] + (M, b, c),
    # and the sliver (a, b, M) [zero area] closes the gap to the neighbour across a-b.  Rule: a zero-area face is measured as
    # its segments and has the normal 0.  The surface is the same set of points: same distances, same signs, no NaN.
    a, b, cc = f[0]
    M = len(v)
    v2 = np.concatenate([v, v[a:a + 1]])
    f2 = np.concatenate([[[a, M, cc], [M, b, cc], [a, b, M]], f[1:]])
    m = gt_sdf.TriMesh(v2, f2)
    assert m.info()['closed']
    got = _np(m.distance(q, signed=True))
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-13 and ((got > 0) == (want > 0)).all()
    m.close()


def test_through_the_boundary(cases, tmp_path):
    from points2surf_amd import gt_sdf
    data = tmp_path / 'abc_minimal'
    shutil.copytree(GOLDEN, str(data), ignore=shutil.ignore_patterns('05_query_dist'))
    written = gt_sdf.write_query_dist_dir(str(data / '03_meshes'), str(data / '05_query_pts'), str(data / '05_query_dist'))
    assert len(written) == 3
    for name, c in cases.items():
        got = np.load(str(data / '05_query_dist' / (name + '.npy')))
        g = c['g'].astype(np.float64)
        assert got.dtype == np.float32 and got.shape == c['g'].shape
        # the file is the float32 rounding of the device's float64 distances (no fixture distance is clamped), and those
        # meet the issue's per-query bound |d_dev - g| <= |d_model - g| + 1e-8 (also test_against_the_recorded_distances)
        dev = _np(c['mesh'].distance(c['q'][:2000], signed=True))
        assert np.array_equal(got, dev.astype(np.float32))
        assert (np.abs(np.abs(dev) - np.abs(g)) <= np.abs(np.abs(c['d'][:2000]) - np.abs(g)) + 1e-8).all()
        assert ((got > 0) == (g > 0)).all()
    assert gt_sdf.write_query_dist_dir(str(data / '03_meshes'), str(data / '05_query_pts'), str(data / '05_query_dist')) == []
    # the drop-in: get_signed_distance and eval_predictions on the written files
    dropin = os.path.join(REPO, 'points2surf_amd', 'dropin')
    for k in [k for k in sys.modules if k == 'source' or k.startswith('source.')]:
        del sys.modules[k]
    sys.path.insert(0, dropin)
    try:
        import source.sdf as sdf
        import source.base.evaluation as evaluation

        class Mesh:
            pass
        c = cases[SMALLEST]
        mesh = Mesh()
        mesh.vertices, mesh.faces = c['v'], c['f']
        d = sdf.get_signed_distance(mesh, c['q'][:2000].astype(np.float64), 1000)
        assert d.dtype == np.float64 and np.array_equal(d, _np(c['mesh'].distance(c['q'][:2000])))
        mesh.faces = c['f'][1:]
        with pytest.raises(ValueError, match='3 open'):
            sdf.get_signed_distance(mesh, c['q'][:10])
        pred = tmp_path / 'pred'
        pred.mkdir()
        for name in MESHES:
            np.save(str(pred / (name[:-4] + '.xyz.npy')), np.load(str(data / '05_query_dist' / (name + '.npy'))))
        evaluation.eval_predictions(str(pred), str(data / '05_query_dist'), str(tmp_path / 'report.csv'))
        rows = open(str(tmp_path / 'report.csv')).read().strip().split('\n')
        assert len(rows) == 4 and all(float(r.split(',')[1]) == 0.0 for r in rows[1:])
    finally:
        sys.path.remove(dropin)
        for k in [k for k in sys.modules if k == 'source' or k.startswith('source.')]:
            del sys.modules[k]


def test_sdf_error_report(cases, tmp_path):
    import torch
    from points2surf_amd import engine, metrics, synth
    pts = np.load(os.path.join(GOLDEN, '04_pts', SMALLEST[:-4] + '.xyz.npy'))
    w, cfg = synth.make_weights('p2s_max')
    model, cloud, rng = engine.Model(w, cfg), engine.Cloud(pts), engine.Rng(40938661)
    sdf, q = engine.infer_shape(model, cloud, rng, 64, 3)
    rec = tmp_path / 'rec'
    (rec / 'dist_ms').mkdir(parents=True)
    (rec / 'query_pts_ms').mkdir()
    stem = SMALLEST[:-4] + '.xyz.npy'
    np.save(str(rec / 'dist_ms' / stem), sdf.cpu().numpy())
    np.save(str(rec / 'query_pts_ms' / stem), q.cpu().numpy())
    rows = metrics.sdf_error(str(rec), os.path.join(GOLDEN, '03_meshes'), str(tmp_path / 'sdf_error.csv'))
    assert len(rows) == 1 and int(rows[0][2]) == q.shape[0]
    gt = np.clip(_np(cases[SMALLEST]['mesh'].distance(q)), -1, 1)
    err = np.abs(sdf.cpu().numpy().astype(np.float64) - gt)
    lines = open(str(tmp_path / 'sdf_error.csv')).read().split('\n')
    assert len(lines) == 2
    cols = lines[1].split(',')
    assert float(cols[3]) == pytest.approx((err * err).mean(), rel=1e-12) and float(cols[4]) == pytest.approx(err.mean(), rel=1e-12)
    assert float(cols[5]) == err.max()
    assert float(cols[6]) == ((sdf.cpu().numpy() > 0) != (gt > 0)).mean()
    cloud.close()
