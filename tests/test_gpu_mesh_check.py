"""p2s_mesh_check on the device (TriMesh.check, clean --stage check, --sign auto) against the CPU model
(tests/mesh_check_model.py): the report slot for slot apart from the candidate counter, the pairs, their classes and the
flags; the walk of the octree against the exhaustive kernel; the capacity rule; the command lines."""
import csv
import ctypes
import os

import numpy as np
import pytest

import clean_model
import mesh_check_model as M
import mesh_sdf_model
from test_mesh_check_model import CASES
from test_mesh_sdf_model import MESHES, load

pytestmark = pytest.mark.gpu

P2S_EINVAL = -1
BUILT = dict(CASES)
BUILT['pierced_grid'] = (lambda: M.pierced_grid(24),)
BUILT['ribbon_prism'] = (M.ribbon_prism,)
# meshes where the index MUST hand over fewer candidates than all pairs: many faces, few of them near each other.  On the
# constructions of two faces whose one pair intersects both kernels test that one pair, so there only "not more" can hold.
STRICTLY_FEWER = {'pierced_grid', 'ribbon_prism'} | set(MESHES)


def _np(t):
    return t.cpu().numpy()


def _check(mesh, method):
    rep, pairs, cls, ff, vf = mesh.check(method=method, want_pairs=True, want_flags=True)
    return rep, _np(pairs), _np(cls), _np(ff), _np(vf)


def _mesh(name):
    if name in BUILT:
        v, f = BUILT[name][0]()
    else:
        v, f = load(name)[:2]
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def _both(name):
    """index == exhaustive, everything but the candidate counter; returns the index's result"""
    from points2surf_amd import gt_sdf
    v, f = _mesh(name)
    mesh = gt_sdf.TriMesh(v, f)
    try:
        a, b = _check(mesh, 'index'), _check(mesh, 'exhaustive')
        assert mesh.check() == a[0]                        # the report alone is the same report
    finally:
        mesh.close()
    other = gt_sdf.TriMesh(v, f)                           # a second handle of the same mesh
    try:
        c = _check(other, 'index')
    finally:
        other.close()
    print(name, 'candidates index', a[0]['candidates'], 'exhaustive', b[0]['candidates'], a[0])
    for k in gt_sdf.CHECK_KEYS:
        assert k == 'candidates' or a[0][k] == b[0][k], (k, a[0], b[0])
    for x, y, z in zip(a[1:], b[1:], c[1:]):
        assert x.dtype == y.dtype and np.array_equal(x, y) and np.array_equal(x, z)
    assert a[0] == c[0]
    assert a[0]['candidates'] <= b[0]['candidates']
    if name in STRICTLY_FEWER:
        assert a[0]['candidates'] < b[0]['candidates']
    p = a[1].astype(np.int64)
    assert a[1].dtype == np.int32 and a[2].dtype == np.uint8 and len(p) == a[0]['pairs_stored']
    assert (p[:, 0] < p[:, 1]).all() and (np.diff(p[:, 0] * len(f) + p[:, 1]) > 0).all()
    return a


def _against_model(name, got):
    v, f = _mesh(name)
    want = M.check(v, f)
    for k in M.REPORT_KEYS:
        assert k == 'candidates' or got[0][k] == want['report'][k], (k, got[0], want['report'])
    assert np.array_equal(got[1], want['pairs']) and np.array_equal(got[2], want['classes'])
    assert np.array_equal(got[3], want['face_flags']) and np.array_equal(got[4], want['vert_flags'])
    return want


@pytest.mark.parametrize('name', sorted(BUILT))
def test_constructions_match_the_model(name):
    want = _against_model(name, _both(name))
    if name in CASES:
        r = want['report']
        assert (r['intersecting'], r['coplanar'], r['touching'], r['nonmanifold_vertices']) == CASES[name][1:]


@pytest.mark.parametrize('name', MESHES)
def test_fixtures_index_equals_exhaustive(name):
    got = _both(name)
    if name.startswith('00994122'):
        _against_model(name, got)                          # 4 M pair tests in numpy blocks
    if name.startswith('00011084'):                        # a union of two overlapping solids
        assert got[0]['pairs_across_components'] > 0
        # the count inside one component is the exhaustive kernel's: _both compared the two slot for slot


def test_capacity_one_short_writes_nothing():
    import torch
    from points2surf_amd import _lib, engine, gt_sdf
    v, f = M.ribbon_prism()
    mesh = gt_sdf.TriMesh(v, f)
    try:
        need = mesh.check()['pairs_stored']
        assert need > 1
        pairs = torch.full((need, 2), -7, dtype=torch.int32, device=mesh.device)
        cls = torch.full((need,), 99, dtype=torch.uint8, device=mesh.device)
        ff = torch.full((len(f),), 77, dtype=torch.uint8, device=mesh.device)
        vf = torch.full((len(v),), 55, dtype=torch.uint8, device=mesh.device)
        rep = (ctypes.c_int64 * 16)()
        for method in (0, 1):
            rc = mesh.lib.p2s_mesh_check(mesh.handle, method, need - 1, engine._ptr(pairs), engine._ptr(cls), engine._ptr(ff),
                                         engine._ptr(vf), rep, engine._stream_ptr(mesh.device))
            assert rc == P2S_EINVAL and rep[11] == need and b'needed' in mesh.lib.p2s_last_error()
            torch.cuda.synchronize()
            assert (pairs == -7).all() and (cls == 99).all() and (ff == 77).all() and (vf == 55).all()
        with pytest.raises(_lib.P2SError):
            mesh.check(want_pairs=True, cap_pairs=need - 1)
        rep2, p2, c2 = mesh.check(want_pairs=True, cap_pairs=need)
        assert len(p2) == need and rep2['pairs_stored'] == need
    finally:
        mesh.close()


def test_open_mesh_has_no_component_counts():
    from points2surf_amd import gt_sdf
    v, f = clean_model.cube()
    f = f[2:]                                              # without its lid
    mesh = gt_sdf.TriMesh(v, f)
    try:
        assert not mesh.closed
        got = _check(mesh, 'index')
    finally:
        mesh.close()
    want = M.check(v, f)
    assert got[0]['pairs_inside_component'] == -1 and got[0]['pairs_across_components'] == -1
    assert {k: got[0][k] for k in M.REPORT_KEYS if k != 'candidates'} == {k: want['report'][k] for k in M.REPORT_KEYS if k != 'candidates'}
    assert np.array_equal(got[1], want['pairs']) and np.array_equal(got[2], want['classes'])
    # and an open mesh WITH pairs: the pierced square
    assert _both('pierced_grid')[0]['pairs_inside_component'] == -1


def _dataset(tmp_path, meshes, queries=None):
    from points2surf_amd import ply
    d = str(tmp_path)
    os.makedirs(os.path.join(d, '03_meshes'))
    os.makedirs(os.path.join(d, '05_query_pts'))
    for name, (v, f) in meshes.items():
        ply.write_ply(os.path.join(d, '03_meshes', name + '.ply'), v, f)
        if queries is not None:
            np.save(os.path.join(d, '05_query_pts', name + '.ply.npy'), queries[name])
    return d


def _dist_files(d):
    out = {}
    for n in sorted(os.listdir(os.path.join(d, '05_query_dist'))):
        with open(os.path.join(d, '05_query_dist', n), 'rb') as fh:
            out[n] = fh.read()
    return out


def test_sign_auto(tmp_path, capsys):
    from points2surf_amd import gt_sdf
    rng = np.random.RandomState(3)
    meshes = {'cube': clean_model.cube(-0.4, 0.4), 'prism': M.ribbon_prism()}
    queries = {'cube': rng.uniform(-0.5, 0.5, (300, 3)).astype(np.float32),
               'prism': np.concatenate([M.RIBBON_QUERIES, rng.uniform(-0.5, 0.5, (276, 3)).astype(np.float32)])}
    files = {}
    for sign in gt_sdf.SIGNS:
        d = _dataset(tmp_path / sign, meshes, queries)
        capsys.readouterr()
        gt_sdf.main(['--indir', d, '--sign', sign])
        out = capsys.readouterr().out
        files[sign] = _dist_files(d)
        switched = [l for l in out.splitlines() if 'signed by the winding number' in l]
        assert len(switched) == (1 if sign == 'auto' else 0) and all('prism.ply' in l for l in switched)
    assert sorted(files['auto']) == ['cube.ply.npy', 'prism.ply.npy']
    assert files['auto']['cube.ply.npy'] == files['pseudonormal']['cube.ply.npy']
    assert files['auto']['prism.ply.npy'] == files['winding']['prism.ply.npy']
    assert files['auto']['prism.ply.npy'] != files['pseudonormal']['prism.ply.npy']
    # the fixed queries: inside by the winding model; the pseudonormal, unchanged, writes them outside
    v, f = meshes['prism']
    mm = mesh_sdf_model.MeshModel(v, f)
    n = len(M.RIBBON_QUERIES)
    inside = np.abs(mesh_sdf_model.winding(M.RIBBON_QUERIES.astype(np.float64), mm.tri)) > 0.5
    assert inside.all()
    auto = np.load(os.path.join(str(tmp_path / 'auto'), '05_query_dist', 'prism.ply.npy'))
    pseudo = np.load(os.path.join(str(tmp_path / 'pseudonormal'), '05_query_dist', 'prism.ply.npy'))
    assert ((auto[:n] > 0) == inside).all() and (pseudo[:n] < 0).all()
    assert np.array_equal(np.abs(auto), np.abs(pseudo))
    # the Python entry points take it too
    mesh = gt_sdf.TriMesh(v, f)
    try:
        assert gt_sdf.auto_sign(mesh)[0] == 'winding'
        assert np.array_equal(gt_sdf.query_dist(mesh, M.RIBBON_QUERIES, sign='auto'), auto[:n])
    finally:
        mesh.close()


def _tree(d):
    out = {}
    for root, _, names in os.walk(d):
        for n in names:
            with open(os.path.join(root, n), 'rb') as fh:
                out[os.path.relpath(os.path.join(root, n), d)] = fh.read()
    return out


def test_stage_check_and_stage_all_unchanged(tmp_path):
    from points2surf_amd import clean, ply
    meshes = {'cube': clean_model.cube(-0.5, 0.5), 'prism': M.ribbon_prism(), 'bowtie': M.bowtie()}
    d = _dataset(tmp_path / 'a', meshes)
    clean.main(['--indir', d, '--stage', 'check'])
    with open(os.path.join(d, clean.CHECK_REPORT_FILE)) as fh:
        rows = {r['mesh']: r for r in csv.DictReader(fh)}
    assert {k: r['verdict'] for k, r in rows.items()} == {'cube.ply': 'embedded', 'prism.ply': 'self-intersecting',
                                                          'bowtie.ply': 'non-manifold'}
    for name, (v, f) in meshes.items():
        want = M.check(v, f)['report']
        assert all(int(rows[name + '.ply'][k]) == want[k] for k in M.REPORT_KEYS if k != 'candidates')
    # --stage all writes what it wrote: the same files with the same bytes whether or not the check stage ran beside it
    trees = []
    for sub, with_check in (('b', False), ('c', True)):
        e = str(tmp_path / sub)
        os.makedirs(os.path.join(e, clean.DIR_BASE))
        for name, (v, f) in meshes.items():
            ply.write_ply(os.path.join(e, clean.DIR_BASE, name + '.ply'), v, f)
        clean.main(['--indir', e, '--stage', 'all'])
        if with_check:
            clean.main(['--indir', e, '--stage', 'check'])
        trees.append(_tree(e))
    extra = trees[1].pop(clean.CHECK_REPORT_FILE)
    assert extra and trees[0] == trees[1]
    assert os.path.join(clean.DIR_CLEANED, clean.REPORT_FILE) in trees[0] and clean.CHECK_REPORT_FILE not in trees[0]
