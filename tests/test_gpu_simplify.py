"""Quadric vertex clustering on the device (p2s_mesh_simplify; points2surf_amd/simplify.py) against the numpy model
(tests/simplify_model.py): the discrete outputs and the mean placement bit for bit, the quadric placement to one float32
ulp, the geometric bounds that hold by construction, the edge cases, and the command line on a temporary directory.

Meshes: the rotated torus of 160 x 64 quads (20,480 faces), the welded unit cube of 24 x 24 quads per side (its lattice lies
on cell boundaries) and the iso-surface of a 32^3 golden volume (its vertices lie on the volume's grid lines)."""
import ctypes
import csv
import functools
import os

import numpy as np
import pytest

import simplify_model as SM

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
P2S_EINVAL = -1
PAD = 4096
RESOLUTIONS = (1, 2, 13, 32, 64, 1024)
MESH_NAMES = ('torus', 'cube', 'iso32')
REPORT_EXACT = (0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 12, 13, 14, 15)


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == 'torus':
        return SM.torus()
    if name == 'cube':
        return SM.cube(24)
    import torch
    from points2surf_amd import engine
    vol = np.load(os.path.join(GOLDEN, 'ref_volume_grid32.npz'))['p2s_max_s5_t13']
    v, f, _ = engine.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).cuda())
    torch.cuda.synchronize()
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert f.shape[0] > 1000
    return v, f


@functools.lru_cache(maxsize=None)
def model(name, resolution, placement, max_faces=0):
    v, f = mesh(name)
    return SM.simplify(v, f, max_faces=max_faces, resolution=resolution, placement=placement)


_HANDLES = {}


def trimesh(name):
    from points2surf_amd import gt_sdf
    if name not in _HANDLES:
        _HANDLES[name] = gt_sdf.TriMesh(*mesh(name))
    return _HANDLES[name]


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for m in _HANDLES.values():
        m.close()
    _HANDLES.clear()


def device(v, f, resolution=0, max_faces=0, placement='quadric', epsilon=1e-3, cap_verts=None, cap_faces=None, expect=0):
    """the raw call with every output filled with a pattern first and PAD entries of it behind; returns numpy arrays"""
    import torch
    from points2surf_amd import _lib, engine, simplify
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    V, F = len(v), len(f)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    cv = V if cap_verts is None else cap_verts
    cf = F if cap_faces is None else cap_faces
    vo = torch.full((3 * cv + PAD,), 77.0, dtype=torch.float32, device=dev)
    fo = torch.full((3 * cf + PAD,), -77, dtype=torch.int32, device=dev)
    so = torch.full((cf + PAD,), -77, dtype=torch.int32, device=dev)
    mo = torch.full((V + PAD,), -77, dtype=torch.int32, device=dev)
    rep = (ctypes.c_int64 * 16)()

    def ptr(t):
        return engine._ptr(t) if t.numel() else None

    rc = lib.p2s_mesh_simplify(ptr(tv), V, ptr(tf), F, resolution, max_faces, simplify.PLACEMENTS[placement], ctypes.c_double(epsilon),
                               engine._ptr(vo), cv, engine._ptr(fo), engine._ptr(so), cf, engine._ptr(mo), rep, dev.index,
                               engine._stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.p2s_last_error().decode())
    vo, fo, so, mo, rep = vo.cpu().numpy(), fo.cpu().numpy(), so.cpu().numpy(), mo.cpu().numpy(), np.array(list(rep), np.int64)
    if rc != 0:
        assert (vo == 77.0).all() and (fo == -77).all() and (so == -77).all() and (mo == -77).all()      # nothing written
        return dict(report=rep, message=lib.p2s_last_error().decode())
    nv, nf = int(rep[1]), int(rep[2])
    assert nv <= cv and nf <= cf
    assert (vo[3 * nv:] == 77.0).all() and (fo[3 * nf:] == -77).all() and (so[nf:] == -77).all() and (mo[V:] == -77).all()
    return dict(verts=vo[:3 * nv].reshape(-1, 3), faces=fo[:3 * nf].reshape(-1, 3), face_src=so[:nf], vert_map=mo[:V], report=rep)


def same_discrete(got, want, fields=REPORT_EXACT):
    assert np.array_equal(got['faces'], want['faces']) and np.array_equal(got['face_src'], want['face_src'])
    assert np.array_equal(got['vert_map'], want['vert_map'])
    for k in fields:
        assert got['report'][k] == want['report'][k], (k, got['report'].tolist(), want['report'].tolist())
    assert got['verts'].shape == want['verts'].shape


def geometric_bounds(name, got, want):
    """every output vertex within h of its cell's centre in the max norm (the fallback rule), and within 1.5 sqrt(3) h of
    the input surface (a cell with an output vertex holds an input vertex within sqrt(3) h / 2 of its centre)"""
    if got['verts'].shape[0] == 0:
        return 0.0, 0.0
    h = want['h']
    off = np.abs(got['verts'].astype(np.float64) - want['centre']).max() / h
    assert off <= 1.0, off
    d = float(trimesh(name).distance(got['verts'], signed=False).max().item())
    assert d <= 1.5 * np.sqrt(3.0) * h * (1.0 + 1e-6), (d, h)
    return off, d / h


@pytest.mark.parametrize('R', RESOLUTIONS)
@pytest.mark.parametrize('name', MESH_NAMES)
def test_device_equals_the_model(name, R):
    """R = 1024: cell ids up to 2^30 - 1; the torus at R = 64: thousands of occupied cells in the table (probing)"""
    v, f = mesh(name)
    # mean placement: equal bytes
    want = model(name, R, 'mean')
    got = device(v, f, resolution=R, placement='mean')
    same_discrete(got, want, REPORT_EXACT + (8, 10))
    assert got['verts'].tobytes() == want['verts'].tobytes()
    off_m, d_m = geometric_bounds(name, got, want)
    # quadric placement: one float32 ulp, except where the fallback decision is within 1e-6 of flipping (no such cell here)
    want = model(name, R, 'quadric')
    got = device(v, f, resolution=R, placement='quadric')
    same_discrete(got, want)
    ratio = want['ratio']
    near = np.abs(ratio - 1.0) <= 1e-6
    assert not near.any(), ratio[near]
    assert got['report'][8] == want['report'][8] and got['report'][10] == want['report'][10]
    a, b = got['verts'].astype(np.float64), want['verts'].astype(np.float64)
    ulp = 2.0 ** -23 * np.maximum(np.abs(b), 2.0 ** -126)
    worst = float((np.abs(a - b) / ulp).max()) if a.size else 0.0
    differ = int((got['verts'].view(np.uint32) != want['verts'].view(np.uint32)).sum())
    off_q, d_q = geometric_bounds(name, got, want)
    r = got['report']
    print('%s R = %d: %d -> %d vertices, %d -> %d faces, %d occupied cells, %d duplicates; quadric %d / tr 0 %d / fallback %d, '
          'largest max|x|/h %.3f; %d of %d coordinates differ from the model, at most %.2f ulp; centre offset %.3f / %.3f h, '
          'distance to the input %.3f / %.3f h (mean / quadric); edges out %d | %d'
          % (name, R, len(v), r[1], len(f), r[2], r[4], r[6], r[8], r[9], r[10], np.nanmax(ratio) if np.isfinite(ratio).any() else 0.0,
             differ, a.size, worst, off_m, off_q, d_m, d_q, r[12] & 0xffffffff, r[12] >> 32))
    assert worst <= 1.0


@pytest.mark.parametrize('name', MESH_NAMES)
def test_the_search_finds_the_models_resolution(name):
    v, f = mesh(name)
    for max_faces in (0, 500, len(f) // 4, len(f) - 1):
        want = model(name, 0, 'quadric', max_faces)
        got = device(v, f, resolution=0, max_faces=max_faces)
        same_discrete(got, want, REPORT_EXACT + (8, 10))
        assert got['report'][11] == 10 and got['report'][2] <= max_faces and 1 <= got['report'][3] <= 1024
        print('%s, at most %d faces: R = %d, %d faces' % (name, max_faces, got['report'][3], got['report'][2]))
    # nothing to do: the input bytes, unreferenced vertices too
    v2 = np.concatenate([v, [[3.0, 3.0, 3.0]]]).astype(np.float32)
    for max_faces in (len(f), len(f) + 1):
        got = device(v2, f, resolution=0, max_faces=max_faces)
        assert got['verts'].tobytes() == v2.tobytes() and got['faces'].tobytes() == f.tobytes()
        assert np.array_equal(got['vert_map'], np.arange(len(v2))) and np.array_equal(got['face_src'], np.arange(len(f)))
        want = SM.simplify(v2, f, max_faces=max_faces)
        assert got['report'].tolist() == want['report'].tolist()


def test_two_runs_give_equal_bytes():
    v, f = mesh('torus')
    a, b = device(v, f, resolution=64), device(v, f, resolution=64)
    for k in ('verts', 'faces', 'face_src', 'vert_map', 'report'):
        assert a[k].tobytes() == b[k].tobytes(), k
    a, b = device(v, f, max_faces=3000), device(v, f, max_faces=3000)
    for k in ('verts', 'faces', 'face_src', 'vert_map', 'report'):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_the_cube_corners_through_the_device():
    v, f = mesh('cube')
    for R in (6, 8):
        q = device(v, f, resolution=R, placement='quadric')
        m = device(v, f, resolution=R, placement='mean')
        h = 1.0 / R
        dq, dm = SM.corner_distances(q['verts'], h), SM.corner_distances(m['verts'], h)
        print('R = %d: corners at %.4f .. %.4f h (quadric), %.3f .. %.3f h (mean)' % (R, dq.min(), dq.max(), dm.min(), dm.max()))
        assert (dq < 0.01).all(), dq
        assert (dm > 0.1).all(), dm
        assert q['report'][8] == q['report'][1] and q['report'][9] == 0 and q['report'][10] == 0


def _both(v, f, **kw):
    """device == model on a small mesh, both placements; returns the device's quadric result"""
    for placement in ('mean', 'quadric'):
        want = SM.simplify(v, f, placement=placement, **kw)
        got = device(v, f, placement=placement, **kw)
        same_discrete(got, want, tuple(range(16)))
        if placement == 'mean' or want['report'][8] == 0:
            assert got['verts'].tobytes() == want['verts'].tobytes()
    return got


def test_edge_cases():
    tri = np.array([[0, 1, 2]], np.int32)
    # ext = 0: every vertex in cell 0, every face collapses
    flat = np.full((3, 3), 0.25, np.float32)
    for R in (1, 7, 1024):
        got = _both(flat, tri, resolution=R)
        assert (got['report'][1], got['report'][2], got['report'][4], got['report'][5]) == (0, 0, 1, 1)
        assert got['vert_map'].tolist() == [-1, -1, -1]
    got = _both(flat, tri, resolution=0, max_faces=0)
    assert got['report'][3] == 1024 and got['report'][2] == 0       # no grid leaves a face: the search ends at its upper end
    # n_faces = 0, with and without vertices
    v, _ = SM.torus(12, 6)
    got = _both(v, np.zeros((0, 3), np.int32), resolution=8)
    assert got['report'].tolist() == [len(v)] + [0, 0, 8] + [0] * 12 and (got['vert_map'] == -1).all()
    got = _both(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), resolution=0, max_faces=5)
    assert got['report'].tolist() == [0] * 16
    # all faces collapsed: R = 1 on a mesh with an extent
    v, f = SM.torus(12, 6)
    got = _both(v, f, resolution=1)
    assert (got['report'][1], got['report'][2], got['report'][4], got['report'][5]) == (0, 0, 1, len(f))
    # degenerate faces only: tr(A) = 0 gives the mean
    line = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1], [0.02, 0.02, 0.02], [0.25, 0.25, 0.25]], np.float32)
    lf = np.array([[0, 1, 2], [3, 1, 2], [4, 2, 0], [1, 1, 2]], np.int32)
    got = _both(line, lf, resolution=4)
    mean = device(line, lf, resolution=4, placement='mean')
    assert got['report'][7] == 4 and got['report'][8] == 0 and got['report'][9] == got['report'][1] > 0
    assert got['verts'].tobytes() == mean['verts'].tobytes()
    # duplicate sets keep the smallest face id; boundary and non-manifold edges of the output are counted
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1], [0.01, 0.01, 0.0], [0.98, 0.0, 0.02]], np.float32)
    f = np.array([[3, 1, 2], [0, 1, 2], [2, 4, 5], [1, 0, 2], [0, 4, 1], [5, 2, 0]], np.int32)
    got = _both(v, f, resolution=2)
    assert got['face_src'].tolist() == [0, 1] and (got['report'][5], got['report'][6]) == (1, 3)
    assert got['report'][12] == 4 and got['report'][13] == SM.edge_word(f)


def test_invalid_input_and_small_buffers_write_nothing():
    v, f = mesh('torus')
    g = f.copy()
    g[5, 1] = len(v)
    assert 'index' in device(v, g, resolution=8, expect=P2S_EINVAL)['message']
    g[5, 1] = -1
    device(v, g, resolution=0, max_faces=10, expect=P2S_EINVAL)
    w = v.copy()
    w[2, 2] = np.nan
    assert 'non-finite' in device(w, f, resolution=8, expect=P2S_EINVAL)['message']
    w[2, 2] = np.inf
    device(w, f, resolution=8, expect=P2S_EINVAL)
    # the capacity: exactly what is needed suffices, one less is refused with the whole report and nothing written
    want = model('torus', 13, 'quadric')
    nv, nf = int(want['report'][1]), int(want['report'][2])
    got = device(v, f, resolution=13, cap_verts=nv, cap_faces=nf)
    same_discrete(got, want)
    for cv, cf in ((nv - 1, nf), (nv, nf - 1), (0, 0)):
        r = device(v, f, resolution=13, cap_verts=cv, cap_faces=cf, expect=P2S_EINVAL)
        assert r['report'].tolist() == got['report'].tolist()
        assert 'cap_verts = %d' % cv in r['message'] and '%d vertices and %d faces needed' % (nv, nf) in r['message']
    r = device(v, f, resolution=0, max_faces=len(f), cap_verts=len(v) - 1, expect=P2S_EINVAL)      # the copy needs room too
    assert (r['report'][1], r['report'][2]) == (len(v), len(f))


def test_python_layer_and_command_line(tmp_path):
    from points2surf_amd import ply, simplify
    v, f = mesh('torus')
    vo, fo, rep = simplify.simplify(v, f, max_faces=2000, want_map=True)
    want = model('torus', 0, 'quadric', 2000)
    assert np.array_equal(fo.cpu().numpy(), want['faces']) and np.array_equal(rep['vert_map'].cpu().numpy(), want['vert_map'])
    assert np.array_equal(rep['face_src'].cpu().numpy(), want['face_src'])
    assert rep['faces_out'] == len(fo) <= 2000 and rep['resolution'] == want['report'][3] and rep['probes'] == 10
    assert rep['boundary_edges_in'] == 0 and rep['nonmanifold_edges_in'] == 0
    indir, outdir = tmp_path / 'in', tmp_path / 'out'
    indir.mkdir()
    ply.write_ply(str(indir / 'torus.ply'), v, f)
    cv, cf = mesh('cube')
    with open(str(indir / 'cube.off'), 'w') as fh:
        fh.write('OFF\n%d %d 0\n' % (len(cv), len(cf)))
        fh.writelines('%r %r %r\n' % tuple(float(x) for x in p) for p in cv)
        fh.writelines('3 %d %d %d\n' % tuple(t) for t in cf)
    (indir / 'broken.ply').write_bytes(b'ply\nformat ascii 1.0\nelement vertex 3\n')
    (indir / 'notes.txt').write_text('not a mesh')
    simplify.main(['--indir', str(indir), '--outdir', str(outdir), '--max_faces', '1500'])
    rows = list(csv.DictReader(open(str(outdir / simplify.REPORT_FILE))))
    assert [r['mesh'] for r in rows] == ['broken.ply', 'cube.off', 'torus.ply']
    assert rows[0]['verdict'].startswith('failed: ') and not (outdir / 'broken.ply').exists()
    for r, (name, n_in) in zip(rows[1:], (('cube', len(cf)), ('torus', len(f)))):
        assert r['verdict'] == 'written' and int(r['faces_in']) == n_in and float(r['milliseconds']) > 0
        vv, ff = ply.read_ply(str(outdir / (name + '.ply')))
        assert len(ff) == int(r['faces_out']) <= 1500 and len(vv) == int(r['verts_out'])
        m = model(name, 0, 'quadric', 1500)
        assert np.array_equal(np.asarray(ff), m['faces']) and int(r['resolution']) == m['report'][3]
