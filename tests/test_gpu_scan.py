"""Ray casting, time-of-flight scan and query points on the device (p2s_mesh_raycast, p2s_mesh_tof_scan,
p2s_mesh_query_points; points2surf_amd/scan.py) against the float64 CPU model (tests/scan_model.py), the exhaustive
kernel, the existing distance kernel and the layout of the reference's recorded data (tests/golden/abc_minimal)."""
import math
import os
import shutil

import numpy as np
import pytest

import mesh_sdf_model as msm
import scan_model as sm
from test_gpu_dropin import _write_model_files, dropin_source          # noqa: F401  (fixture)
from test_mesh_sdf_model import GOLDEN, MESHES, load

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALLEST = '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.ply'
RECORDED = {'00011084': 59979, '00016513': 86648, '00994122': 34693}      # points of the reference's own 04_pts clouds
TW, TH = math.tan(math.radians(43.6) / 2.0), math.tan(math.radians(34.6) / 2.0)


def _np(t):
    return t.cpu().numpy()


def _random_rays(v, f, q, g, seed, n=20000):
    """seeded rays: from outside towards the mesh, origins inside the mesh, along the coordinate axes, aimed exactly at
    vertices and at edge midpoints, and a few that are no rays at all"""
    rs = np.random.RandomState(seed)
    v64 = v.astype(np.float64)
    k = n // 5
    o = rs.uniform(-2.0, 2.0, (n, 3))
    d = rs.standard_normal((n, 3))
    d[:k] = rs.uniform(-0.5, 0.5, (k, 3)) - o[:k]                       # towards the mesh
    inside = q[g > 0].astype(np.float64)
    o[k:2 * k] = inside[rs.randint(0, len(inside), k)]                  # origins inside the mesh
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    ax = axes[rs.randint(0, 6, k)]                                      # along the axes (half of them through a vertex)
    o[2 * k:3 * k] = np.where(rs.rand(k, 1) < 0.5, o[2 * k:3 * k], v64[rs.randint(0, len(v64), k)] - 3.0 * ax)
    d[2 * k:3 * k] = ax
    d[3 * k:4 * k] = v64[rs.randint(0, len(v64), k)] - o[3 * k:4 * k]   # at vertices
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    mid = v64[e[rs.randint(0, len(e), n - 4 * k)]]
    d[4 * k:] = (mid[:, 0] + mid[:, 1]) * 0.5 - o[4 * k:]               # at edge midpoints
    rays = np.concatenate([o, d], 1)
    rays[0, 3:] = 0.0
    rays[1, 0] = np.nan
    rays[2, 4] = np.inf
    rays[3, 2] = 1e301
    rays[4, 3:] = [1e-310, -5e-324, 0.0]                                # only subnormal components: no direction
    rays[5, 3] = 1e-310                                                 # one subnormal component: counts as 0
    return rays


@pytest.fixture(scope='module')
def cases():
    from points2surf_amd import scan
    out = {}
    for name in MESHES:
        v, f, q, g = load(name)
        T = sm.triangles(v, f)
        poses = scan.scan_poses(name)
        out[name] = dict(v=v, f=f, q=q, g=g, T=T, poses=poses, mesh=scan.TriMesh(v, f),
                         scan_rays=sm.scan_rays(poses['locations'], poses['rotations'], 176, 144, TW, TH),
                         rays=_random_rays(v, f, q, g, len(f)))
    yield out
    for c in out.values():
        c['mesh'].close()


def test_index_equals_exhaustive_bit_for_bit(cases):
    from points2surf_amd import scan
    for name, c in cases.items():
        m = c['mesh']
        assert len(c['scan_rays']) == c['poses']['n_scans'] * 176 * 144 and len(c['rays']) == 20000
        for label, rays, t_max in (('scan', c['scan_rays'], 10.0), ('random', c['rays'], float('inf')), ('random<=2', c['rays'], 2.0)):
            ti, fi = (_np(x) for x in m.raycast(rays, t_max, method='index'))
            tests = m.ray_tests
            te, fe = (_np(x) for x in m.raycast(rays, t_max, method='exhaustive'))
            print(name[:8], label, 'rays', len(rays), 'hits', int((fi >= 0).sum()), 'tests per ray', tests / len(rays), 'of', len(c['f']))
            assert not np.isnan(ti).any() and not np.isnan(te).any()
            assert np.array_equal(ti, te) and np.array_equal(fi, fe), (name, label)
            assert np.array_equal(fi < 0, np.isinf(ti)) and (ti[fi >= 0] > 0).all() and (ti[fi >= 0] <= t_max).all()
            assert 0 < tests < len(rays) * len(c['f'])
        assert (fi[:5] == -1).all()                                       # zero direction, NaN, inf, beyond 1e300, subnormal
        # the scan through the tiled launch: the same hits as the plain launch, both methods
        a = scan.tof_scan(m, c['poses'], method='index')
        b = scan.tof_scan(m, c['poses'], method='exhaustive')
        for key in ('points', 'points_noisefree', 'normals', 'face'):
            assert np.array_equal(_np(a[key]), _np(b[key])), (name, key)
        assert np.array_equal(a['hits_per_scan'], b['hits_per_scan'])
        ts, fs = (_np(x) for x in m.raycast(c['scan_rays'], 10.0))
        assert np.array_equal(_np(a['face']), fs[fs >= 0])
        assert np.array_equal(a['hits_per_scan'], (fs >= 0).reshape(c['poses']['n_scans'], -1).sum(1))


def test_exhaustive_kernel_against_the_cpu_model(cases):
    """The device and the model perform the same correctly rounded float64 operations (+ - x /) in the same association
    with contraction off: t is expected bit-identical, and the face identical wherever the model's runner-up differs in
    t.  Rays: 1,500 of the random rays (every class of them) and 1,500 of the mesh's own scan rays."""
    for name, c in cases.items():
        rs = np.random.RandomState(3)
        rays = np.concatenate([c['rays'][:6], c['rays'][rs.permutation(20000)[:1494]],
                               c['scan_rays'][rs.permutation(len(c['scan_rays']))[:1500]]])
        t, face, second = sm.cast(c['T'], rays, 10.0)
        td, fd = (_np(x) for x in c['mesh'].raycast(rays, 10.0, method='exhaustive'))
        both = np.isfinite(t) & np.isfinite(td)
        diff = np.abs(td[both] - t[both])
        print(name[:8], 'model hits', int(np.isfinite(t).sum()), 'device hits', int(np.isfinite(td).sum()),
              'max |t dev - t model|', diff.max() if len(diff) else 0.0, 'ties', int((second == t)[np.isfinite(t)].sum()))
        assert np.array_equal(td, t), name
        clear = second != t
        assert np.array_equal(fd[clear], face[clear]), name


def test_hits_agree_with_the_distance_kernel(cases):
    """every noise-free hit lies on the mesh for the distance kernel: the queries are float32, every fixture coordinate
    is below 1 in magnitude, so rounding moves a point by at most sqrt(3) 2^-25 = 1.03e-7 < 2e-7.  The nearest face is the
    hit face, or ties with it in distance: the squared distance of the rounded point to the hit face (model, float64)
    is not above the device's squared distance to the face it returned by more than 1e-13, the bound within which
    device and model agree on d^2 (test_gpu_mesh_sdf.py)."""
    from points2surf_amd import scan
    for name, c in cases.items():
        r = scan.tof_scan(c['mesh'], c['poses'])
        p32 = _np(r['points_noisefree']).astype(np.float32)
        hit_face = _np(r['face'])
        d, near = (_np(x) for x in c['mesh'].distance(p32, signed=False, want_face=True))
        other = np.nonzero(near != hit_face)[0]
        print(name[:8], 'hits', len(p32), 'max distance', d.max(), 'nearest face differs', len(other))
        assert d.max() <= 2e-7
        if len(other):
            d2, _, _ = msm.tri_closest(p32[other].astype(np.float64), c['T'][hit_face[other]])
            print('   max (d2 hit face - d2 nearest)', (d2 - d[other] ** 2).max())
            assert (d2 <= d[other] ** 2 + 1e-13).all()


def test_scan_semantics_against_the_model(cases):
    from points2surf_amd import _lib, scan
    sensor = dict(width=24, height=20, angle_w=43.6, angle_h=34.6, max_distance=10.0)
    for name, c in cases.items():
        p = c['poses']
        loc = np.concatenate([p['locations'][:3], [[0.0, -4.0, 0.0]]])          # the last pose has the object behind the camera
        rot = np.concatenate([p['rotations'][:3], [[1.0, 0.0, 0.0, 0.0]]])
        g = np.random.RandomState(5).standard_normal(4 * 24 * 20)
        poses = dict(locations=loc, rotations=rot, sigma=0.01, noise=g)
        want = sm.tof_scan(c['T'], loc, rot, 0.01, g, 24, 20, TW, TH, 10.0)
        for method in ('index', 'exhaustive'):
            got = scan.tof_scan(c['mesh'], poses, sensor=sensor, method=method)
            print(name[:8], method, 'hits per scan', got['hits_per_scan'], 'model', want['hits_per_scan'])
            assert got['hits_per_scan'].dtype == np.int32 and np.array_equal(got['hits_per_scan'], want['hits_per_scan'])
            assert got['hits_per_scan'][3] == 0 and got['hits_per_scan'][:3].min() > 0
            clear = (want['second'] != want['t'])[want['face_all'] >= 0]
            assert np.array_equal(_np(got['face'])[clear], want['face'][clear])         # the compaction order
            assert np.array_equal(_np(got['points_noisefree']), want['points_noisefree'])
            assert np.array_equal(_np(got['points']), want['points'])                  # o + (t + sigma g) d, as the model
            # the handle's stored normals: n * (1 / sqrt(n . n)), correctly rounded operations in the model's association
            assert np.array_equal(_np(got['normals'])[clear], want['normals'][clear])
        zero = scan.tof_scan(c['mesh'], dict(poses, sigma=0.0), sensor=sensor)
        assert np.array_equal(_np(zero['points']), _np(zero['points_noisefree']))
        assert np.array_equal(_np(zero['points_noisefree']), want['points_noisefree'])
        away = scan.tof_scan(c['mesh'], dict(locations=loc[3:], rotations=rot[3:], sigma=0.01, noise=g[:480]), sensor=sensor)
        assert away['hits_per_scan'].tolist() == [0] and away['tests'] >= 0
        for key in ('points', 'points_noisefree', 'normals'):
            assert tuple(away[key].shape) == (0, 3)
        assert tuple(away['face'].shape) == (0,)
        with pytest.raises(_lib.P2SError, match='unit quaternion') as ei:
            scan.tof_scan(c['mesh'], dict(poses, rotations=rot * [[1.0], [1.0], [1.0 + 1e-12], [1.0]]), sensor=sensor)
        assert ei.value.code == -1
        none = scan.tof_scan(c['mesh'], dict(locations=np.zeros((0, 3)), rotations=np.zeros((0, 4)), sigma=0.0, noise=np.zeros(0)), sensor=sensor)
        assert tuple(none['points'].shape) == (0, 3) and len(none['hits_per_scan']) == 0


def _meshes_only(tmp_path):
    data = tmp_path / 'abc_minimal'
    os.makedirs(str(data / '03_meshes'))
    for name in MESHES:
        shutil.copy(os.path.join(GOLDEN, '03_meshes', name), str(data / '03_meshes' / name))
    return data


def test_files(cases, tmp_path, dropin_source):
    from points2surf_amd import ply, scan
    ev, _ = dropin_source
    data = _meshes_only(tmp_path)
    written = scan.write_pts_dir(str(data))
    assert len(written) == 3
    for name in MESHES:
        stem = name[:-4]
        ref = np.load(os.path.join(GOLDEN, '04_pts', stem + '.xyz.npy'))
        pts = np.load(str(data / '04_pts' / (stem + '.xyz.npy')))
        clean = np.load(str(data / '04_pts_noisefree' / (stem + '.xyz.npy')))
        nrm = np.load(str(data / '06_normals' / 'pts' / (stem + '.xyz.npy')))
        hits = np.load(str(data / '04_hits_per_scan' / (stem + '.xyz.npz')))['hits_per_scan']
        loc = np.load(str(data / '04_locations' / (stem + '.npz')))['locations']
        rot = np.load(str(data / '04_rotations' / (stem + '.npz')))['rotations']
        print('%s: %d points in %d scans (the reference recorded %d)' % (stem[:8], len(pts), len(hits), RECORDED[stem[:8]]))
        assert len(ref) == RECORDED[stem[:8]]
        for a in (pts, clean, nrm):
            assert a.dtype == ref.dtype == np.float32 and a.ndim == ref.ndim == 2 and a.shape == (len(pts), 3) and np.isfinite(a).all()
        assert hits.dtype == np.int32 and hits.sum() == len(pts) > 1000
        p = cases[name]['poses']
        assert np.array_equal(loc, p['locations']) and np.array_equal(rot, p['rotations']) and len(hits) == p['n_scans']
        assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-6
        assert np.abs(pts).max() < 1.0 + 6 * p['sigma']
        loaded = ev._load_points(str(data), stem)
        assert np.array_equal(loaded, pts) and loaded.flags['C_CONTIGUOUS']
    assert scan.write_pts_dir(str(data)) == []
    # an open mesh is refused
    bad = tmp_path / 'open'
    os.makedirs(str(bad / '03_meshes'))
    c = cases[SMALLEST]
    ply.write_ply(str(bad / '03_meshes' / 'open.ply'), c['v'], c['f'][1:])
    with pytest.raises(ValueError, match='3 open or non-manifold edges'):
        scan.write_pts_dir(str(bad))
    with pytest.raises(ValueError, match='3 open or non-manifold edges'):
        scan.write_query_pts_dir(str(bad), 4.0 / 256)
    assert not os.path.exists(str(bad / '04_pts')) and not os.path.exists(str(bad / '05_query_pts'))


def test_query_points(cases, tmp_path):
    from points2surf_amd import gt_sdf, scan
    r = 4.0 / 256
    for name, c in cases.items():
        seed = scan.filename_to_hash(name)
        pts, samples, fid = scan.query_points(c['mesh'], seed, 2000, r, want_parts=True)
        q = _np(pts)
        assert q.dtype == np.float32 and q.shape == (2000, 3)
        assert (q[:200] >= -0.5).all() and (q[:200] < 0.5).all()
        rs = np.random.RandomState(seed)
        rs.random_sample(3 * 1800)
        u_off, u_far = rs.random_sample(1800), rs.random_sample(600)
        # the construction, on the device's own samples: equal to the model
        want, off = sm.query_points_from(_np(samples), _np(fid), sm.face_normals(c['T']), u_off, u_far, r)
        assert np.array_equal(q, want)
        # the whole of it against the model's own surface samples.  The device picks a face by a parallel scan of the
        # areas, the model by np.cumsum: a pick may land on another face only if it lies within the rounding of a sum of F
        # areas (F 2^-52 of the total) of the cumulative boundary between the two; everything else is equal
        full, samples_m, face_m, off_m = sm.query_points(c['v'], c['f'], seed, 2000, r)
        assert np.array_equal(off_m, off) and np.array_equal(q[:200], full[:200])
        same = _np(fid) == face_m
        tri = c['v'].astype(np.float64)[c['f']]
        cum = np.cumsum(np.sqrt((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(1)) / 2.0)
        pick = np.random.RandomState(seed).random_sample(1800) * cum[-1]
        lo_f = np.minimum(_np(fid), face_m)[~same]
        print(name[:8], 'faces picked differently from np.cumsum:', int((~same).sum()), 'of 1800')
        assert (np.abs(pick[~same] - cum[lo_f]) <= len(cum) * 2.0 ** -52 * cum[-1]).all()
        # on the same face the device's sample is the model's float64 expression in another order of summation, rounded
        # to float32: equal, or one float32 ulp apart across a rounding boundary (2^-24, coordinates below 1); the query
        # point adds the same offset and rounds once more: at most a second ulp, 2^-23
        dm = np.abs(q[200:][same].astype(np.float64) - full[200:][same])
        print(name[:8], 'max |dev - full model| on the same faces', dm.max(), 'unequal', int((dm > 0).any(1).sum()))
        assert dm.max() <= 2.0 ** -23
        d = _np(c['mesh'].distance(q[200:], signed=False))
        print(name[:8], 'max (distance - |offset|)', (d - np.abs(off)).max())
        assert (d <= np.abs(off) + 2e-7).all()
        again = _np(scan.query_points(c['mesh'], seed, 2000, r))
        assert np.array_equal(again, q)
    data = _meshes_only(tmp_path)
    written = scan.write_query_pts_dir(str(data), r)
    assert len(written) == 3 and scan.write_query_pts_dir(str(data), r) == []
    for name, c in cases.items():
        q = np.load(str(data / '05_query_pts' / (name + '.npy')))
        assert q.dtype == np.float32 and q.shape == (2000, 3)
        assert np.array_equal(q, _np(scan.query_points(c['mesh'], scan.filename_to_hash(name), 2000, r)))
    dist = gt_sdf.write_query_dist_dir(str(data / '03_meshes'), str(data / '05_query_pts'), str(data / '05_query_dist'))
    assert len(dist) == 3
    for f in dist:
        d = np.load(f)
        assert d.dtype == np.float32 and d.shape == (2000,) and np.isfinite(d).all() and (np.abs(d) <= 1.0).all()
        assert (d > 0).any() and (d < 0).any()


def test_chain_from_meshes_to_evaluation(tmp_path, dropin_source):
    """meshes -> scan -> gt_sdf -> the drop-in's evaluation pass at 32^3 on the scanned cloud (synthetic weights: the pass
    completes and writes its files; no accuracy is asserted)"""
    from points2surf_amd import gt_sdf, scan
    ev, _ = dropin_source
    data = tmp_path / 'ds'
    os.makedirs(str(data / '03_meshes'))
    shutil.copy(os.path.join(GOLDEN, '03_meshes', SMALLEST), str(data / '03_meshes' / SMALLEST))
    (data / 'settings.ini').write_text('[general]\nonly_for_evaluation = 0\ngrid_resolution = 256\nepsilon = 3\n'
                                       'num_scans_per_mesh_min = 5\nnum_scans_per_mesh_max = 6\n'
                                       'scanner_noise_sigma_min = 0.0\nscanner_noise_sigma_max = 0.01\n')
    (data / 'testset.txt').write_text(SMALLEST[:-4] + '\n')
    scan.main(['--indir', str(data)])
    gt_sdf.main(['--indir', str(data)])
    stem = SMALLEST[:-4]
    pts = np.load(str(data / '04_pts' / (stem + '.xyz.npy')))
    hits = np.load(str(data / '04_hits_per_scan' / (stem + '.xyz.npz')))['hits_per_scan']
    assert 5 <= len(hits) <= 6 and hits.sum() == len(pts) > 1000
    assert np.load(str(data / '05_query_dist' / (SMALLEST + '.npy'))).shape == (2000,)
    modeldir, outdir = str(tmp_path / 'models'), str(tmp_path / 'results')
    _write_model_files(modeldir, 'p2s_max')
    opt = ev.parse_arguments(['--indir', str(data), '--outdir', outdir, '--dataset', 'testset.txt', '--modeldir', modeldir,
                              '--models', 'p2s_max', '--query_grid_resolution', '32', '--epsilon', '3',
                              '--certainty_threshold', '13', '--sigma', '5'])
    opt.reconstruction = True
    ev.points_to_surf_eval(opt)
    sdf = np.load(os.path.join(outdir, 'rec', 'dist_ms', stem + '.xyz.npy'))
    q = np.load(os.path.join(outdir, 'rec', 'query_pts_ms', stem + '.xyz.npy'))
    assert len(sdf) == len(q) > 0 and np.isfinite(sdf).all()
    assert os.path.isfile(os.path.join(outdir, 'rec', 'eval', stem + '.xyz.npy'))
