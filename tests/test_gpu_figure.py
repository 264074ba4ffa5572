"""p2s_mesh_render on the device (points2surf_amd/figure.py) against the numpy model (tests/figure_model.py) for EQUALITY: the
image bytes, the depth bits, the face ids and stats[0..5]; nothing written beyond the outputs; depth and face against
TriMesh.raycast on the same rays; partial tiles and a lone lane; sample tiles that straddle pixels; ties on a cube's edges and
diagonals; an open sheet from behind; the smooth fallback at a degenerate face; an inward-oriented mesh (stored flipped) with
a colour per vertex; a camera inside; a view of nothing; occlusion rays that hit and miss within one wave; an occlusion radius
shorter than the bias; determinism; the refusals; the command line."""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest

import figure_model as FM

pytestmark = pytest.mark.gpu

P2S_EINVAL = -1
PAD = 256


def _dev():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def _colours(n, seed, lo=0.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def _mesh(name):
    if name == 'ico1280':
        return FM.icosphere(3)
    if name == 'ico320':
        return FM.icosphere(2)
    if name == 'ico80_inward':
        v, f = FM.icosphere(1)
        return v, np.ascontiguousarray(f[:, [0, 2, 1]])
    if name == 'cube3':
        return FM.cube(3.0)
    if name == 'sheet':
        return FM.sheet(4, 1.0)
    if name == 'ico80_degenerate':                   # a second vertex at the place of vertex 0: a zero-area face, three flagged vertices
        v, f = FM.icosphere(1)
        return np.concatenate([v, v[0:1]]), np.concatenate([f, np.array([(0, 1, len(v))], np.int32)])
    if name == 'floor_plate':
        return FM.floor_and_plate(0.25, 0.5)
    raise KeyError(name)


def _case(mesh, colours=None, table_seed=None, **kw):
    return dict(mesh=mesh, colours=colours, table_seed=table_seed, p=FM.params(**kw))


S = 2.0 ** -0.5
CASES = {
    # the octree has levels (G = 16); 13 x 11 pixels: partial tiles; ss = 2
    'ico1280_pinhole_flat_k5': _case('ico1280', width=13, height=11, samples=2, ao_rays=5, ao_radius=0.6, tan_half_w=0.45, tan_half_h=0.4),
    'ico1280_ortho_smooth_k1': _case('ico1280', colours=(-0.5, 1.5), width=9, height=40, samples=1, ao_rays=1, projection=1, shading=1,
                                     half_w=1.1, half_h=1.2, ao_radius=0.3, **FM.look_at((2.0, 1.0, 2.0), (0.0, 0.0, 0.0))),
    # a lone lane, alone and with a 3 x 3 sample tile
    'lone_pixel': _case('ico320', width=1, height=1, samples=1, ao_rays=0),
    'lone_pixel_ss3_k5': _case('ico320', width=1, height=1, samples=3, ao_rays=5, shading=1, tan_half_w=0.3, tan_half_h=0.3, ao_radius=0.5),
    # ss = 3: the 8 x 8 sample tiles straddle pixels (39 x 33 samples)
    'ico320_ss3_smooth': _case('ico320', colours=(0.0, 1.0), width=13, height=11, samples=3, ao_rays=1, shading=1, tan_half_w=0.45,
                               tan_half_h=0.4, ao_radius=0.5, **FM.look_at((1.0, 2.0, 2.0), (0.0, 0.1, 0.0))),
    # sample rays at the odd integers -7 .. 7 in x and y: exactly on the cube's edges (x, y = +-3), its corners, and the diagonal of its top
    'cube_ties_flat': _case('cube3', width=8, height=8, samples=1, ao_rays=5, projection=1, eye=(0.0, 0.0, 9.0), half_w=8.0, half_h=8.0,
                            ao_radius=2.0),
    'cube_ties_smooth': _case('cube3', colours=(0.0, 1.0), width=8, height=8, samples=1, ao_rays=0, projection=1, shading=1, eye=(0.0, 0.0, 9.0),
                              half_w=8.0, half_h=8.0),
    'cube_edge_on': _case('cube3', width=9, height=40, samples=1, ao_rays=1, projection=1, ao_radius=1.0, half_w=6.0, half_h=6.0,
                          **FM.look_at((9.0, 0.0, 9.0), (0.0, 0.0, 0.0))),
    # an open sheet from behind: the normal is flipped toward the camera, the occlusion rays leave on the camera's side
    'sheet_from_behind': _case('sheet', colours=(0.0, 1.0), width=13, height=11, samples=3, ao_rays=1, tan_half_w=0.5, tan_half_h=0.45,
                               ao_radius=0.5, **FM.look_at((0.3, 0.2, -3.0), (0.0, 0.0, 0.0))),
    'degenerate_smooth_fallback': _case('ico80_degenerate', width=13, height=11, samples=2, ao_rays=1, shading=1, tan_half_w=0.45,
                                        tan_half_h=0.4, ao_radius=0.5, **FM.look_at((-1.0, 2.5, 1.0), (0.0, 0.0, 0.0))),
    # stored flipped: the colours must still land on the right corners
    'inward_flat': _case('ico80_inward', colours=(0.0, 1.0), width=13, height=11, samples=2, ao_rays=1, tan_half_w=0.45, tan_half_h=0.4,
                         ao_radius=0.5),
    'inward_smooth': _case('ico80_inward', colours=(0.0, 1.0), width=13, height=11, samples=2, ao_rays=0, shading=1, tan_half_w=0.45,
                           tan_half_h=0.4),
    'camera_inside': _case('ico320', width=9, height=40, samples=1, ao_rays=5, tan_half_w=0.5, tan_half_h=2.0, ao_radius=0.8,
                           **FM.look_at((0.1, 0.2, 0.0), (1.0, 0.0, 0.3))),
    'ico1280_inside_k5': _case('ico1280', width=13, height=11, samples=1, ao_rays=5, shading=1, tan_half_w=0.8, tan_half_h=0.7, ao_radius=0.8,
                               **FM.look_at((0.2, -0.1, 0.3), (1.0, 0.5, 0.0))),
    'view_of_nothing': _case('ico320', width=13, height=11, samples=2, ao_rays=5, **FM.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 9.0))),
    'colours_at_0_and_1': _case('ico320', colours='zero_one', width=13, height=11, samples=1, ao_rays=0, tan_half_w=0.45, tan_half_h=0.4,
                                ambient=0.7, diffuse=0.9),
    'radius_shorter_than_bias': _case('floor_plate', width=13, height=11, samples=1, ao_rays=5, ao_radius=1.0 / 1024.0, ao_bias=1.0 / 64.0,
                                      tan_half_w=0.6, tan_half_h=0.5, **FM.look_at((1.0, -4.0, 3.0), (0.0, 0.0, 0.0))),
    'radius_zero': _case('floor_plate', width=8, height=8, samples=1, ao_rays=1, ao_radius=0.0, ao_bias=0.0, tan_half_w=0.6, tan_half_h=0.5,
                         **FM.look_at((1.0, -4.0, 3.0), (0.0, 0.0, 0.0))),
    # 40 x 30: the floor around the plate, where some occlusion rays of a wave reach the plate and others do not
    'floor_under_plate': _case('floor_plate', width=40, height=30, samples=1, ao_rays=5, ao_radius=0.75, tan_half_w=0.6, tan_half_h=0.45,
                               **FM.look_at((1.0, -4.0, 3.0), (0.0, 0.0, 0.0))),
    'floor_under_plate_random_table': _case('floor_plate', table_seed=5, width=13, height=11, samples=2, ao_rays=5, ao_radius=0.75, shading=1,
                                            tan_half_w=0.6, tan_half_h=0.45, **FM.look_at((1.0, -4.0, 3.0), (0.0, 0.0, 0.0))),
}


def _inputs(case):
    from points2surf_amd import figure
    v, f = _mesh(case['mesh'])
    c = case['colours']
    if c == 'zero_one':
        col = (np.arange(3 * len(v)).reshape(-1, 3) % 2).astype(np.float32)
    else:
        col = _colours(len(v), 7, *c) if c else None
    K = case['p']['ao_rays']
    table = figure.ao_directions(K) if K else None
    if K and case['table_seed'] is not None:         # any unit directions of the upper hemisphere will do
        t = np.random.RandomState(case['table_seed']).normal(size=(K, 3))
        t[:, 2] = np.abs(t[:, 2])
        table = t / np.sqrt((t * t).sum(1))[:, None]
    return v, f, col, table


@functools.lru_cache(maxsize=None)
def model(name):
    v, f, col, table = _inputs(CASES[name])
    return FM.render(v, f, CASES[name]['p'], vertex_rgb=col, ao_dirs=table)


@functools.lru_cache(maxsize=None)
def device_mesh(name):
    from points2surf_amd import scan
    v, f = _mesh(name)
    return scan.TriMesh(v, f)


def raw_render(mesh, p, col=None, table=None, want_depth=True, want_face=True, host=()):
    """the raw call with the three outputs filled with a pattern first and PAD entries of it behind; ``host`` names the
    pointers passed as host addresses -> rc, rgb, depth, face, stats"""
    import torch
    from points2surf_amd import _lib, engine
    from points2surf_amd.figure import PROJECTIONS, SHADINGS, render_params
    dev = _dev()
    W, H, ss = p['width'], p['height'], p['samples']
    n = max(W, 0) * max(H, 0) * ss * ss
    cam = dict(p, projection=PROJECTIONS[p['projection']]) if p['projection'] in (0, 1) else None
    if cam is not None and p['shading'] in (0, 1):
        prm = render_params(cam, W, H, ss, p['ao_rays'], SHADINGS[p['shading']], p['ao_radius'], p['ao_bias'], p['ambient'], p['diffuse'],
                            p['base_rgb'], p['background_rgb'])
    else:
        prm = render_params(dict(p, projection='pinhole'), W, H, ss, p['ao_rays'], 'flat', p['ao_radius'], p['ao_bias'], p['ambient'],
                            p['diffuse'], p['base_rgb'], p['background_rgb'])
        prm.projection, prm.shading = p['projection'], p['shading']
    rgb = np.full(3 * max(W, 0) * max(H, 0) + PAD, 0xAB, np.uint8)
    depth, face = np.full(n + PAD, -77.0), np.full(n + PAD, -55, np.int32)
    keep = [np.ascontiguousarray(col, np.float32) if col is not None else None, np.ascontiguousarray(table, np.float64) if table is not None else None]
    t = {}
    for key, a in (('vrgb', keep[0]), ('dirs', keep[1]), ('rgb', rgb), ('depth', depth if want_depth else None), ('face', face if want_face else None)):
        t[key] = None if a is None else (a if key in host else torch.from_numpy(a).to(dev))
    ptr = lambda x: None if x is None else (ctypes.c_void_p(x.ctypes.data) if isinstance(x, np.ndarray) else engine._ptr(x))
    stats = (ctypes.c_int64 * 8)(*([-1] * 8))
    rc = _lib.load().p2s_mesh_render(mesh.handle, ctypes.byref(prm), ptr(t['vrgb']), ptr(t['dirs']), ptr(t['rgb']), ptr(t['depth']), ptr(t['face']),
                                     stats, engine._stream_ptr(dev))
    torch.cuda.synchronize()
    back = lambda x, a: a if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy())
    return rc, back(t['rgb'], rgb), back(t['depth'], depth), back(t['face'], face), np.array(stats[:], np.int64)


def untouched(got):
    return np.all(got[1] == 0xAB) and np.all(got[2] == -77.0) and np.all(got[3] == -55) and np.all(got[4] == -1)


def check(m, got, want_depth=True, want_face=True):
    rc, rgb, depth, face, stats = got
    H, W = m['rgb'].shape[:2]
    n = m['depth'].size
    assert rc == 0
    print('stats device %s model %s' % (stats.tolist(), m['stats'].tolist()))
    assert rgb[:3 * W * H].tobytes() == m['rgb'].tobytes() and np.all(rgb[3 * W * H:] == 0xAB)
    assert depth[:n].tobytes() == m['depth'].tobytes() if want_depth else np.all(depth == -77.0)
    assert np.all(depth[n:] == -77.0)
    assert face[:n].tobytes() == m['face'].tobytes() if want_face else np.all(face == -55)
    assert np.all(face[n:] == -55)
    assert stats[:6].tolist() == m['stats'][:6].tolist() and stats[6:].tolist() == [0, 0]


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_model(name):
    case, m = CASES[name], model(name)
    _, _, col, table = _inputs(case)
    mesh = device_mesh(case['mesh'])
    assert mesh.info()['inverted'] == m['inverted']
    check(m, raw_render(mesh, case['p'], col, table))
    t, f = mesh.raycast(m['rays'])                                   # the primary pass IS the ray unit's, bit for bit
    assert t.cpu().numpy().tobytes() == m['depth'].tobytes() and f.cpu().numpy().tobytes() == m['face'].tobytes()


def test_the_cases_cover_what_they_claim():
    assert model('view_of_nothing')['stats'][1] == 0 and not (model('view_of_nothing')['rgb'] != 255).any()
    inside = model('camera_inside')
    assert inside['stats'][1] == inside['stats'][0] and inside['stats'][3] > 0
    floor = model('floor_under_plate')
    occ = 1.0 - floor['ao'].reshape(30, 40)
    tiles = [occ[y:y + 8, x:x + 8] for y in range(0, 30, 8) for x in range(0, 40, 8)]
    assert any((t > 0).any() and (t == 0).any() for t in tiles)      # hits and misses within one wave
    assert model('radius_shorter_than_bias')['stats'][3] == 0 and model('radius_shorter_than_bias')['stats'][2] > 0
    assert model('radius_zero')['stats'][3] == 0
    ties = model('cube_ties_flat')
    face = ties['face']                                              # x = 2 i - 7, y = 7 - 2 j: the top's diagonal x = y belongs to both of its faces
    assert (face >= 0).sum() == 16 and set(face[face >= 0].tolist()) == {10, 11}
    assert [face[5, 2], face[4, 3], face[3, 4], face[2, 5]] == [10] * 4 and face[2, 2] == 11
    assert model('inward_flat')['inverted'] and model('inward_flat')['stats'][1] > 50
    v, f = _mesh('ico80_degenerate')
    from mesh_sdf_model import MeshModel
    mm = MeshModel(v, f)
    smooth = model('degenerate_smooth_fallback')
    seen = np.unique(smooth['face'][smooth['face'] >= 0])
    flagged = mm.vbad[mm.faces[seen]].any(1)
    assert mm.vbad.sum() == 3 and flagged.any() and not flagged.all()          # faces that fall back and faces that do not are in view
    hit = smooth['face'].reshape(-1) >= 0
    fell = np.zeros(len(hit), bool)
    fell[hit] = mm.vbad[mm.faces[smooth['face'].reshape(-1)[hit]]].any(1)
    n = smooth['normal']
    flat_n = mm.fn[smooth['face'].reshape(-1)[fell]]
    assert np.array_equal(np.abs(n[fell]), np.abs(flat_n)) and not np.array_equal(np.abs(n[hit & ~fell]), np.abs(mm.fn[smooth['face'].reshape(-1)[hit & ~fell]]))
    wide = model('ico1280_ortho_smooth_k1')
    assert (wide['colour'] == 0.0).any() and (wide['colour'] == 1.0).any()      # colours outside [0, 1] reach the clamp


def test_outputs_may_be_null_and_two_runs_agree():
    name = 'ico320_ss3_smooth'
    case, m = CASES[name], model(name)
    _, _, col, table = _inputs(case)
    mesh = device_mesh(case['mesh'])
    first = raw_render(mesh, case['p'], col, table)
    for want_depth, want_face in ((False, True), (True, False), (False, False), (True, True)):
        got = raw_render(mesh, case['p'], col, table, want_depth, want_face)
        check(m, got, want_depth, want_face)
        assert got[1].tobytes() == first[1].tobytes() and got[4].tolist() == first[4].tolist()


def test_render_wrapper_returns_the_same_arrays():
    from points2surf_amd import figure
    name = 'ico1280_pinhole_flat_k5'
    p, m = CASES[name]['p'], model(name)
    cam = dict(p, projection=figure.PROJECTIONS[p['projection']])
    kw = dict(camera=cam, width=p['width'], height=p['height'], samples=p['samples'], ao_rays=p['ao_rays'], ao_radius=p['ao_radius'],
              ao_bias=p['ao_bias'], ambient=p['ambient'], diffuse=p['diffuse'], base_rgb=p['base_rgb'], background_rgb=p['background_rgb'])
    rgb, depth, face, st = figure.render(device_mesh('ico1280'), want_depth=True, want_face=True, want_stats=True, **kw)
    assert rgb.tobytes() == m['rgb'].tobytes() and depth.tobytes() == m['depth'].tobytes() and face.tobytes() == m['face'].tobytes()
    assert [st[k] for k in figure.STATS_KEYS] == m['stats'][:6].tolist()
    assert figure.render(_mesh('ico1280'), **kw).tobytes() == m['rgb'].tobytes()          # from (verts, faces)
    auto = figure.render(device_mesh('ico1280'), width=16, height=12, samples=1, ao_rays=2)       # the fitted camera sees all of it
    assert auto.shape == (12, 16, 3) and (auto != 255).any() and (auto[0] == 255).all() and (auto[:, 0] == 255).all()


BAD = [dict(width=0), dict(height=-1), dict(samples=0), dict(samples=5), dict(ao_rays=65), dict(projection=2), dict(shading=-1),
       dict(eye=(float('nan'), 0.0, 3.0)), dict(tan_half_w=0.0), dict(ao_radius=float('inf')), dict(ambient=float('nan')),
       dict(base_rgb=(0.5, float('inf'), 0.5)), dict(right=(S, S, 0.0)), dict(up=(0.0, 1.0 + 2.0 ** -30, 0.0)), dict(ao_radius=-0.5),
       dict(ao_bias=-0.5)]


@pytest.mark.parametrize('bad', BAD + ['no_table', 'table_without_rays', 'host_rgb', 'host_depth', 'host_face', 'host_table', 'host_colours'])
def test_refusals_leave_the_outputs_untouched(bad):
    from points2surf_amd import _lib, figure
    mesh = device_mesh('ico320')
    v, _ = _mesh('ico320')
    p, col, table, host = FM.params(width=13, height=11, samples=2, ao_rays=5), _colours(len(v), 3), figure.ao_directions(5), ()
    if isinstance(bad, dict):
        p = dict(p, **bad)
    elif bad == 'no_table':
        table = None
    elif bad == 'table_without_rays':
        p = dict(p, ao_rays=0)
    else:
        host = ({'host_rgb': 'rgb', 'host_depth': 'depth', 'host_face': 'face', 'host_table': 'dirs', 'host_colours': 'vrgb'}[bad],)
    got = raw_render(mesh, p, col, table, host=host)
    msg = _lib.load().p2s_last_error().decode()
    assert got[0] == P2S_EINVAL and 'p2s_mesh_render' in msg, (got[0], msg)
    assert untouched(got)
    if host:
        assert dict(rgb='rgb_out_dev', depth='depth_out_dev', face='face_out_dev', dirs='ao_dirs_dev', vrgb='vertex_rgb_dev')[host[0]] in msg


def test_command_line(tmp_path):
    from points2surf_amd import figure, ply, scan
    names = ('a_sphere', 'b_cube', 'c_fine')
    gts = dict(zip(names, (FM.icosphere(1), FM.cube(0.4), FM.icosphere(2, 0.5))))
    gt_dir, recs = tmp_path / 'gt_meshes', (tmp_path / 'method_one', tmp_path / 'method_two')
    for d in (gt_dir,) + recs:
        d.mkdir()
    rng = np.random.RandomState(11)
    made = {}
    for name, (v, f) in gts.items():
        ply.write_ply(str(gt_dir / (name + '.ply')), v, f)
        for k, d in enumerate(recs):
            rv = (v * (1.02 + 0.03 * k) + rng.normal(0.0, 0.01, v.shape)).astype(np.float32)
            ply.write_ply(str(d / (name + '.ply')), rv, f)
            made[(d.name, name)] = (rv, f)
    (recs[1] / 'unpaired.ply').write_bytes((recs[1] / 'a_sphere.ply').read_bytes())          # no GT of that name: not rendered
    out = tmp_path / 'out'
    opt = dict(width=40, height=30, samples=2, ao_rays=4)
    argv = ['--rec', str(recs[0]), str(recs[1]), '--gt', str(gt_dir), '--outdir', str(out), '--cut', '0.8', '--azimuth', '40', '--elevation', '25']
    for k, x in opt.items():
        argv += ['--' + k, str(x)]
    assert figure.main(argv) == 0
    rows = list(csv.DictReader(open(str(out / figure.REPORT_FILE), newline='')))
    assert len(rows) == 9 and all(r['verdict'] == 'rendered' for r in rows) and tuple(rows[0]) == figure.REPORT_COLUMNS
    assert sorted(r['picture'] for r in rows) == sorted([os.path.join('gt', n + '.png') for n in names] +
                                                        [os.path.join(d.name, n + '.png') for d in recs for n in names])
    for name, (gv, gf) in gts.items():
        gt = scan.TriMesh(gv, gf)
        camera = figure.fit_camera(figure.mesh_bounds(gt), 40.0, 25.0, aspect=40.0 / 30.0)
        ao = dict(ao_radius=0.1 * camera['radius'], ao_bias=camera['radius'] / 1024.0)
        assert FM.decode_png((out / 'gt' / (name + '.png')).read_bytes()).tobytes() == figure.render(gt, camera=camera, **opt, **ao).tobytes()
        dist = [figure.vertex_distances(made[(d.name, name)][0], gt) for d in recs]
        assert all(len(x) == len(gv) and (x >= 0.0).all() and x.max() < 0.2 for x in dist)
        target = figure.normalization_target(dist, 0.8)
        for d, dd in zip(recs, dist):
            rv, rf = made[(d.name, name)]
            base = out / d.name / name
            text = open(str(base) + '_stats.txt').read()
            assert 'normalised to %r (cut 0.8)' % target in text and 'max %r' % float(dd.max()) in text        # one target per group
            pv, pf = ply.read_ply(str(base) + '_vis.ply')
            assert np.array_equal(np.asarray(pv, np.float32), rv) and np.array_equal(np.asarray(pf), rf)
            colours = figure.distance_colors(dd, target)
            raw = open(str(base) + '_vis.ply', 'rb').read()
            body = raw[raw.index(b'end_header\n') + 11:]
            rec = np.frombuffer(body[:16 * len(rv)], dtype=[('p', '<f4', 3), ('c', 'u1', 4)])
            assert np.array_equal(rec['c'][:, :3], colours) and (rec['c'][:, 3] == 255).all()
            want = figure.render((rv, rf), vertex_rgb=figure.linear_albedo(colours), camera=camera, **opt, **ao)
            assert FM.decode_png(open(str(base) + '.png', 'rb').read()).tobytes() == want.tobytes()
            row = [r for r in rows if r['picture'] == os.path.join(d.name, name + '.png')][0]
            assert row['target'] == repr(target) and row['source'] == d.name and int(row['verts']) == len(rv)
        gt.close()
    assert not (out / 'method_two' / 'unpaired.png').exists()
    plain = tmp_path / 'plain'                                        # without --gt: plain pictures, a camera per mesh
    assert figure.main(['--rec', str(recs[0]), '--outdir', str(plain), '--width', '16', '--height', '12', '--samples', '1', '--ao_rays', '0']) == 0
    assert sorted(os.listdir(str(plain / 'method_one'))) == [n + '.png' for n in names]
    assert FM.decode_png((plain / 'method_one' / 'b_cube.png').read_bytes()).shape == (12, 16, 3)
