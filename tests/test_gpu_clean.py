"""The mesh repair and the normalisation on the device (p2s_mesh_repair, p2s_mesh_normalize; points2surf_amd/clean.py)
against the CPU model (tests/clean_model.py): vertices, faces, face_src and the whole report bit for bit.  The soups of the
three fixture meshes come back as the fixtures, and the handle (p2s_trimesh_create) agrees.  The command line on a
temporary data set."""
import ctypes
import os
import struct

import numpy as np
import pytest

import clean_model as M
from test_clean_model import two_cubes_sharing_an_edge, two_holes_one_vertex
from test_mesh_sdf_model import MESHES, load

pytestmark = pytest.mark.gpu

P2S_EINVAL, P2S_EFLAT = -1, -7


def _np(t):
    return t.cpu().numpy()


def _same(v, f, **kw):
    """device == model, everything; returns the device's result as numpy"""
    from points2surf_amd import clean
    want = M.repair(v, f, **kw)
    got = clean.repair(v, f, **kw)
    assert got[3] == want[3]
    vo, fo, so = _np(got[0]), _np(got[1]), _np(got[2])
    assert vo.dtype == np.float32 and fo.dtype == np.int32 and so.dtype == np.int32
    assert np.array_equal(vo.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(fo, want[1]) and np.array_equal(so, want[2])
    return vo, fo, so, got[3]


def _flipped(f, seed, fraction=0.5):
    fl = np.random.RandomState(seed).rand(len(f)) < fraction
    return np.where(fl[:, None], f[:, [0, 2, 1]], f).astype(np.int32)


def _nested_cubes():
    v, f = M.cube()
    v2, f2 = M.cube(0.25, 0.75)
    return np.concatenate([v, v2]), np.concatenate([f, f2[:, [0, 2, 1]] + 8])


def _ico_without_fan():
    v, f = M.icosahedron()
    return v, f[~(f == 0).any(axis=1)]


SMALL = {
    'cube_half_flipped': lambda: (M.cube()[0], _flipped(M.cube()[1], 7)),
    'tetrahedron_inside_out': lambda: (M.tetrahedron()[0], M.tetrahedron()[1][:, [0, 2, 1]]),
    'two_holes_one_vertex': two_holes_one_vertex,
    'moebius': M.moebius,
    'two_cubes_sharing_an_edge': two_cubes_sharing_an_edge,
    'cube_in_cube_inner_inverted': _nested_cubes,
    'single_triangle': lambda: (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)),
    'all_faces_collapse': lambda: (M.cube()[0], np.array([[0, 0, 1], [2, 3, 3], [5, 4, 5]], np.int32)),
    'no_faces': lambda: (M.cube()[0], np.zeros((0, 3), np.int32)),
    'nothing': lambda: (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
}


@pytest.mark.parametrize('name', sorted(SMALL))
def test_device_equals_model(name):
    v, f = SMALL[name]()
    vo, fo, so, r = _same(v, f)
    if name == 'moebius':
        assert np.array_equal(vo, v) and np.array_equal(fo, f) and r['components_unorientable'] == 1
    if name == 'two_cubes_sharing_an_edge':
        assert r['nonmanifold_edges'] == 1 and r['components'] == 2 and not r['watertight']
    if name == 'cube_in_cube_inner_inverted':
        assert r['components_inverted'] == 1 and r['is_volume']
    if name == 'single_triangle':
        assert r['faces_out'] == 2 and r['watertight'] and not r['is_volume']
    if name in ('all_faces_collapse', 'no_faces', 'nothing'):
        assert vo.shape == (0, 3) and fo.shape == (0, 3) and so.shape == (0,)
    if name == 'two_holes_one_vertex':
        assert r['holes_filled'] == 0 and r['boundary_edges_left'] == 6


@pytest.mark.parametrize('k', [4, 3, 0])
def test_cube_holes(k):
    v, f = M.cube()
    r3 = _same(v, f[1:], max_hole_edges=k)[3]
    r4 = _same(v, f[2:], max_hole_edges=k)[3]
    assert r3['holes_filled'] == (k >= 3) and r4['holes_filled'] == (k >= 4) and r4['faces_added'] == (2 if k >= 4 else 0)


def test_five_hole_is_left_at_four_and_filled_at_five():
    v, f = _ico_without_fan()
    assert _same(v, f, max_hole_edges=4)[3]['holes_left'] == 1
    r = _same(v, f, max_hole_edges=5)[3]
    assert r['holes_filled'] == 1 and r['faces_added'] == 3 and r['is_volume']
    assert _same(v, f, max_hole_edges=64)[3] == r


# Face counts one below, at and one above every size at which a kernel of p2s_meshrepair.inl changes its launch or a table
# its capacity (rp_table_cap: the power of two >= max(1024, 2 n)):
#   255 / 256 / 257    one workgroup of 256 threads per 256 faces
#   170 / 171 / 172    the edge table of 3 F half-edges: 6 F passes 1024 at F = 171
#   341 / 342          6 F passes 2048
#   511 / 512 / 513    the face table (2 F passes 1024 at F = 513) and two workgroups
#   682 / 683          6 F passes 4096
#   1280               the closed sphere; as a soup 3840 vertices: the vertex table at 8192
#   1023 / 1024 / 1025 and 2047 / 2048 / 2049    the one-workgroup scan (p2s_scan_kernel) walks its input in chunks of 1024
#                      with a carry: the kept faces [F] and the closed roots [F1] end one below, at and one above the first
#                      and the second chunk; every face survives, so the positions behind the carry are all used (a sphere
#                      cut from 5120 faces keeps its 2562 vertices: the used vertices [V] take three chunks)
SPHERE_FACES = [170, 171, 172, 255, 256, 257, 341, 342, 511, 512, 513, 682, 683, 1280, 1023, 1024, 1025, 2047, 2048, 2049]


@pytest.mark.parametrize('n', SPHERE_FACES)
def test_spheres_at_size_steps(n):
    v, f = M.sphere(n)
    assert len(f) == n
    _same(v, _flipped(f, n, 0.3))
    sv, sf, _ = M.soup(v, f, seed=n, n_duplicate=5, n_collapsed=5)
    r = _same(sv, sf)[3]
    assert r['faces_out'] >= n and (n != 1280 or r['is_volume'])


@pytest.mark.parametrize('n_verts', [511, 512, 513])
def test_vertex_table_step(n_verts):
    # the vertex table (2 V passes 1024 at V = 513): a soup of 150 faces padded with unreferenced vertices
    v, f = M.sphere(150)
    sv, sf, _ = M.soup(v, f, seed=1, n_duplicate=0, n_collapsed=0)
    pad = np.random.RandomState(2).rand(n_verts - len(sv), 3).astype(np.float32)
    _same(np.concatenate([sv, pad]), sf)


@pytest.fixture(scope='module')
def soups():
    """name -> fixture verts, faces, queries, recorded distances, soup verts, soup faces, its injected flips"""
    out = {}
    for i, name in enumerate(MESHES):
        v, f, q, g = load(name)
        invert = None
        if name.startswith('00011084') or name.startswith('00994122'):
            comp = _components(f)
            invert = comp == comp[-1]                   # one whole component inside out
        sv, sf, fl = M.soup(v, f, seed=100 + i, invert=invert)
        out[name] = (v, f, q, g, sv, sf, fl)
    return out


def _components(f):
    parent = list(range(int(f.max()) + 1))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in f.tolist():
        parent[find(a)] = find(b)
        parent[find(b)] = find(c)
    return np.array([find(a) for a in f[:, 0].tolist()])


@pytest.mark.parametrize('name', MESHES)
def test_soup_round_trip(soups, name):
    from points2surf_amd import clean, gt_sdf
    v, f, q, g, sv, sf, fl = soups[name]
    vo, fo, so, r = clean.repair(sv, sf)
    vo, fo, so = _np(vo), _np(fo), _np(so)
    assert np.array_equal(vo[fo], v[f])                 # exactly, as float32, in face order
    assert np.array_equal(so, np.arange(len(f)))
    n_comp = len(set(_components(f).tolist()))
    assert r['verts_in'] == 3 * len(f) + 600 and r['faces_in'] == len(f) + 200
    assert r['verts_out'] == len(v) and r['faces_out'] == len(f) and r['verts_welded'] == 3 * len(f) + 600 - len(v)
    assert r['faces_collapsed'] == 100 and r['faces_duplicate'] == 100 and r['components'] == n_comp
    assert r['holes_filled'] == 0 and r['holes_left'] == 0 and r['boundary_edges_left'] == 0 and r['nonmanifold_edges'] == 0
    assert r['watertight'] and r['winding_consistent'] and r['is_volume'] and r['components_unorientable'] == 0
    # every injected flip is undone, by the orientation or by the inversion of its whole component
    want = M.repair(sv, sf)
    assert r == want[3] and np.array_equal(fo, want[1]) and np.array_equal(vo.view(np.uint32), want[0].view(np.uint32))
    comp = _components(f)
    first = {c: bool(fl[np.flatnonzero(comp == c)[0]]) for c in set(comp.tolist())}      # the flip of each component's first face
    assert r['faces_flipped'] == sum(int((fl[comp == c] != first[c]).sum()) for c in first)     # step d: agree with that face
    assert r['components_inverted'] == sum(first.values())                                  # step f: then turn the whole

    # the handle: the soup is not closed; the repaired mesh is, with the fixture's components, and measures the same
    m_soup = gt_sdf.TriMesh(sv, sf)
    m_rep = gt_sdf.TriMesh(vo, fo)
    m_fix = gt_sdf.TriMesh(v, f)
    try:
        assert not m_soup.info()['closed']
        info = m_rep.info()
        assert info['closed'] and not info['inverted'] and info['components'] == n_comp
        d = _np(m_rep.distance(q, signed=True))
        d_fix = _np(m_fix.distance(q, signed=True))
        assert np.array_equal(np.abs(d).view(np.uint64), np.abs(d_fix).view(np.uint64))
        assert np.array_equal(np.sign(d), np.sign(g))
    finally:
        for m in (m_soup, m_rep, m_fix):
            m.close()


def test_reproducible(soups):
    from points2surf_amd import clean
    sv, sf = soups[MESHES[0]][4:6]
    a, b = clean.repair(sv, sf), clean.repair(sv, sf)
    assert a[3] == b[3]
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(_np(x).view(np.uint32), _np(y).view(np.uint32))


def test_normalize(soups):
    from points2surf_amd import clean
    for name in MESHES:
        v = soups[name][0] * np.float32(37.3) + np.float32([5.0, -80.0, 0.125])
        n = _np(clean.normalize(v))
        assert np.array_equal(n.view(np.uint32), M.normalize(v).view(np.uint32))
        ext = n.max(0).astype(np.float64) - n.min(0).astype(np.float64)
        assert ext.max() == 1.0
        assert np.abs(n.max(0).astype(np.float64) + n.min(0)).max() / 2.0 <= 2.0 ** -24    # the centre: one float32 ulp of the bounds (0.5)
    with pytest.raises(clean.FlatMesh):
        clean.normalize(np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32))


def test_invalid_input_writes_nothing():
    import torch
    from points2surf_amd import _lib, clean, engine
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    v, f = M.cube()

    def call(v, f, k=4, cap_v=None, cap_f=None):
        tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev)
        cv = len(v) if cap_v is None else cap_v
        cf = 4 * len(f) if cap_f is None else cap_f
        vo = torch.full((max(cv, 1), 3), 77.0, dtype=torch.float32, device=dev)
        fo = torch.full((max(cf, 1), 3), 77, dtype=torch.int32, device=dev)
        so = torch.full((max(cf, 1),), 77, dtype=torch.int32, device=dev)
        rep = (ctypes.c_int64 * 16)()
        rc = lib.p2s_mesh_repair(engine._ptr(tv), len(v), engine._ptr(tf), len(f), k, engine._ptr(vo), cv, engine._ptr(fo),
                                 engine._ptr(so), cf, rep, dev.index, engine._stream_ptr(dev))
        torch.cuda.synchronize()
        assert rc == P2S_EINVAL
        assert bool((vo == 77.0).all()) and bool((fo == 77).all()) and bool((so == 77).all())
        return clean.report_dict(rep)

    g = f.copy()
    g[5, 1] = 8
    call(v, g)
    g[5, 1] = -1
    call(v, g)
    w = v.copy()
    w[2, 2] = np.nan
    call(w, f)
    w[2, 2] = np.inf
    call(w, f)
    call(v, f, k=65)
    call(v, f, k=-1)
    r = call(v, f[1:], cap_f=11)                         # the filled hole needs a twelfth face
    assert r['faces_out'] == 12 and r['verts_out'] == 8
    r = call(v, f, cap_v=7)
    assert r['verts_out'] == 8 and r['faces_out'] == 12
    with pytest.raises(_lib.P2SError) as e:
        clean.repair(v, f[1:], cap_faces=11)
    assert e.value.code == P2S_EINVAL
    with pytest.raises(_lib.P2SError):
        clean.normalize(w)


def _write_stl(path, v, f):
    with open(path, 'wb') as fh:
        fh.write(b'soup'.ljust(80, b' ') + struct.pack('<I', len(f)))
        rec = np.zeros(len(f), dtype=np.dtype([('n', '<f4', 3), ('v', '<f4', 9), ('a', '<u2')]))
        rec['v'] = v[f].reshape(len(f), 9)
        fh.write(rec.tobytes())


def _write_off(path, v, f):
    with open(path, 'w') as fh:
        fh.write('OFF\n%d %d 0\n' % (len(v), len(f)))
        fh.write(''.join('%r %r %r\n' % tuple(float(x) for x in p) for p in v))
        fh.write(''.join('3 %d %d %d\n' % tuple(t) for t in f.tolist()))


def test_cli(soups, tmp_path):
    import csv
    from points2surf_amd import clean, gt_sdf, ply, scan
    d = str(tmp_path)
    base = os.path.join(d, clean.DIR_BASE)
    os.makedirs(base)
    for i, name in enumerate(MESHES):
        sv, sf = soups[name][4:6]
        if i == len(MESHES) - 1:
            _write_off(os.path.join(base, name[:-4] + '.off'), sv, sf)
        else:
            _write_stl(os.path.join(base, name[:-4] + '.stl'), sv, sf)
    ov, of = M.sphere(300)                                # 20 faces short of closed: boundaries beyond the limit
    _write_off(os.path.join(base, 'open.off'), ov, of)
    clean.main(['--indir', d, '--stage', 'all'])
    for name in MESHES:
        v, f = soups[name][:2]
        sv, sf = soups[name][4:6]
        pv, pf = ply.read_ply(os.path.join(d, clean.DIR_PLY, name))
        assert np.array_equal(pv.astype(np.float32)[pf], sv[sf])
        cv, cf = ply.read_ply(os.path.join(d, clean.DIR_CLEANED, name))
        assert len(cv) == len(v) and np.array_equal(cv.astype(np.float32)[cf], v[f])      # vertices in the order of their first use
        nv, nf = ply.read_ply(os.path.join(d, clean.DIR_MESHES, name))
        assert np.array_equal(nv.astype(np.float32)[nf], M.normalize(v)[f])
    assert not os.path.exists(os.path.join(d, clean.DIR_CLEANED, 'open.ply'))
    assert not os.path.exists(os.path.join(d, clean.DIR_MESHES, 'open.ply'))
    with open(os.path.join(d, clean.DIR_CLEANED, clean.REPORT_FILE)) as fh:
        rows = {r['mesh']: r for r in csv.DictReader(fh)}
    assert set(rows) == set(MESHES) | {'open.ply'}
    assert rows['open.ply']['verdict'].startswith('rejected: not watertight') and int(rows['open.ply']['holes_left']) == M.repair(ov, of)[3]['holes_left'] >= 1
    assert all(rows[name]['verdict'] == 'written' and rows[name]['is_volume'] == '1' for name in MESHES)
    # the stages behind it accept the result
    assert len(scan.write_query_pts_dir(d, scan.read_settings(d)['patch_radius'], 200)) == len(MESHES)
    gt_sdf.main(['--indir', d])
    for name in MESHES:
        assert np.load(os.path.join(d, '05_query_dist', name + '.npy')).shape == (200,)
    clean.main(['--indir', d, '--stage', 'all', '--no_enforce_solid', '--max_hole_edges', '3'])
    assert os.path.isfile(os.path.join(d, clean.DIR_CLEANED, 'open.ply')) and os.path.isfile(os.path.join(d, clean.DIR_MESHES, 'open.ply'))
    clean.main(['--indir', d, '--stage', 'clean', '--max_faces', '5000'])
    assert sorted(os.listdir(os.path.join(d, clean.DIR_CLEANED))) == sorted(
        [clean.REPORT_FILE] + [n for n in MESHES if len(soups[n][1]) < 5000])
