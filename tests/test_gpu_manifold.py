"""p2s_mesh_manifold on the device (points2surf_amd/manifold.py) against the numpy model (tests/manifold_model.py) for EQUALITY
on every case and every mode: vertices, faces, both source arrays, report [0..10]; nothing written beyond the counts;
determinism; the capacity refusal; agreement with the existing, independent code (p2s_mesh_components counts no edge of more
than two faces in the output, p2s_mesh_check no non-manifold vertex); the output of p2s_mesh_simplify; the command line."""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest

import manifold_model as MM

pytestmark = pytest.mark.gpu

P2S_EINVAL = -1
PAD = 1024
CASES = MM.small_cases()
HAND = sorted(k for k in CASES if not k.startswith('soup'))
SOUPS = sorted(k for k in CASES if k.startswith('soup'))


@functools.lru_cache(maxsize=None)
def big():
    v, f = MM.big_case()
    return v, f, {mode: MM.manifold(v, f, mode) for mode in MM.MODES}


def _dev():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def raw_manifold(v, f, mode, cap_verts=None, cap_faces=None, maps=True):
    """the raw call with every output filled with a pattern first and PAD entries of it behind -> rc, numpy arrays, report"""
    import torch
    from points2surf_amd import _lib, engine
    lib, dev = _lib.load(), _dev()
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    V, F = len(v), len(f)
    cv, cf = 3 * F if cap_verts is None else cap_verts, F if cap_faces is None else cap_faces
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    vo = torch.full((3 * cv + PAD,), 77.0, dtype=torch.float32, device=dev)
    fo = torch.full((3 * cf + PAD,), -77, dtype=torch.int32, device=dev)
    vs = torch.full((cv + PAD,), -77, dtype=torch.int32, device=dev)
    fs = torch.full((cf + PAD,), -77, dtype=torch.int32, device=dev)
    rep = (ctypes.c_int64 * 16)(*([-1] * 16))
    ptr = lambda t, n: engine._ptr(t) if n else None
    rc = lib.p2s_mesh_manifold(ptr(tv, V), V, ptr(tf, F), F, mode, engine._ptr(vo), cv, engine._ptr(fo), cf, engine._ptr(vs) if maps else None,
                               engine._ptr(fs) if maps else None, rep, dev.index, engine._stream_ptr(dev))
    return rc, vo.cpu().numpy(), fo.cpu().numpy(), vs.cpu().numpy(), fs.cpu().numpy(), np.array(rep[:], np.int64)


def check_manifold(m, got, maps=True):
    rc, vo, fo, vs, fs, rep = got
    nv, nf = len(m['verts']), len(m['faces'])
    assert rc == 0
    assert rep[:11].tolist() == m['report'][:11].tolist() and rep[12:].tolist() == [0, 0, 0, 0] and rep[11] >= 0
    assert vo[:3 * nv].tobytes() == m['verts'].tobytes() and np.all(vo[3 * nv:] == 77.0)
    assert np.array_equal(fo[:3 * nf].reshape(-1, 3), m['faces']) and np.all(fo[3 * nf:] == -77)
    if maps:
        assert np.array_equal(vs[:nv], m['vert_src']) and np.all(vs[nv:] == -77)
        assert np.array_equal(fs[:nf], m['face_src']) and np.all(fs[nf:] == -77)
    else:
        assert np.all(vs == -77) and np.all(fs == -77)


def check_independent(vo, fo, mode):
    """the existing units on the output: no edge of more than two faces (components); no non-manifold vertex (mesh check)"""
    from points2surf_amd import components, gt_sdf
    if len(fo) == 0:
        return
    st = components.components(vo, fo)[1]
    assert int(st['nonmanifold_edges'].sum()) == 0
    if mode & 2:
        mesh = gt_sdf.TriMesh(vo, fo)
        try:
            assert mesh.check()['nonmanifold_vertices'] == 0
        finally:
            mesh.close()


@pytest.mark.parametrize('name', HAND)
def test_hand_made_cases(name):
    v, f = CASES[name]
    for mode in MM.MODES:
        m = MM.manifold(v, f, mode)
        check_manifold(m, raw_manifold(v, f, mode))
        check_independent(m['verts'], m['faces'], mode)
        again = raw_manifold(m['verts'], m['faces'], mode)              # idempotent: its own output comes back, the same bytes
        assert again[0] == 0 and again[1][:3 * len(m['verts'])].tobytes() == m['verts'].tobytes()
        assert np.array_equal(again[2][:3 * len(m['faces'])].reshape(-1, 3), m['faces'])


@pytest.mark.parametrize('mode', MM.MODES)
def test_random_soups(mode):
    for name in SOUPS:
        v, f = CASES[name]
        m = MM.manifold(v, f, mode)
        check_manifold(m, raw_manifold(v, f, mode))
        check_independent(m['verts'], m['faces'], mode)


def test_optional_outputs_may_be_null():
    v, f = CASES['octahedra_sharing_two_edges']
    for mode in MM.MODES:
        check_manifold(MM.manifold(v, f, mode), raw_manifold(v, f, mode, maps=False), maps=False)


@pytest.mark.parametrize('mode', MM.MODES)
def test_big_case_and_determinism(mode):
    v, f, want = big()
    a = raw_manifold(v, f, mode)
    check_manifold(want[mode], a)
    print('mode %d: hook rounds %d, report %s' % (mode, a[5][11], a[5][:11].tolist()))
    b = raw_manifold(v, f, mode)
    for x, y in zip(a[1:5], b[1:5]):
        assert x.tobytes() == y.tobytes()
    assert a[5][:11].tolist() == b[5][:11].tolist()
    check_independent(want[mode]['verts'], want[mode]['faces'], mode)


def test_capacity_refusal_fills_the_report_and_writes_nothing():
    from points2surf_amd import manifold
    v, f, want = big()
    for mode in MM.MODES:
        m = want[mode]
        nv, nf = len(m['verts']), len(m['faces'])
        for cv, cf in ((nv - 1, nf), (nv, nf - 1)):
            rc, vo, fo, vs, fs, rep = raw_manifold(v, f, mode, cap_verts=cv, cap_faces=cf)
            assert rc == P2S_EINVAL and rep[:11].tolist() == m['report'][:11].tolist()
            assert np.all(vo == 77.0) and np.all(fo == -77) and np.all(vs == -77) and np.all(fs == -77)
        check_manifold(m, raw_manifold(v, f, mode, cap_verts=nv, cap_faces=nf))
    # the Python call starts below what the split of this mesh needs and repeats with the exact count
    v, f = CASES['book4']
    vo, fo, rep = manifold.manifold(np.tile(v, (1, 1)), np.tile(f, (400, 1)), want_map=True)
    m = MM.manifold(v, np.tile(f, (400, 1)), 2)
    assert rep['verts_out'] == len(m['verts']) > len(v) + len(v) // 8 + 1024
    assert vo.cpu().numpy().tobytes() == m['verts'].tobytes() and np.array_equal(fo.cpu().numpy(), m['faces'])
    assert np.array_equal(rep['vert_src'].cpu().numpy(), m['vert_src']) and np.array_equal(rep['face_src'].cpu().numpy(), m['face_src'])


def test_invalid_meshes_are_refused():
    from points2surf_amd import _lib
    v, f = CASES['book3']
    for bad, word in (([0, 1, 5], b'out of range'), ([0, -1, 2], b'out of range'), ([0, 1, 1], b'repeated'), ([2, 1, 2], b'repeated')):
        g = f.copy()
        g[1] = bad
        got = raw_manifold(v, g, 2)
        assert got[0] == P2S_EINVAL and word in _lib.load().p2s_last_error() and np.all(got[1] == 77.0) and np.all(got[2] == -77)
    nan = v.copy()
    nan[2, 1] = np.nan
    assert raw_manifold(nan, f, 3)[0] == P2S_EINVAL and b'non-finite' in _lib.load().p2s_last_error()


def test_simplified_sheets_lose_their_nonmanifold_edges():
    """two close sheets, simplified on a grid that merges them: report [12] of p2s_mesh_simplify shows edges of more than two
    faces; after manifold they are gone, in every mode"""
    from points2surf_amd import manifold, simplify
    v, f = MM.two_sheets()
    sv, sf, srep = simplify.simplify(v, f, resolution=12, placement='mean')
    assert srep['nonmanifold_edges_out'] > 50
    sv, sf = sv.cpu().numpy(), sf.cpu().numpy()
    assert MM.defects(sf)[0] == srep['nonmanifold_edges_out']
    for edges, split, mode in (('remove', False, 1), ('split', True, 2), ('remove', True, 3)):
        vo, fo, rep = manifold.manifold(sv, sf, edges=edges, split=split)
        m = MM.manifold(sv, sf, mode)
        assert rep['nonmanifold_edges_in'] == srep['nonmanifold_edges_out'] and rep['boundary_edges_in'] == srep['boundary_edges_out']
        assert vo.cpu().numpy().tobytes() == m['verts'].tobytes() and np.array_equal(fo.cpu().numpy(), m['faces'])
        assert MM.defects(fo.cpu().numpy()) == ((0, 0) if split else (0, MM.defects(m['faces'])[1]))
        check_independent(vo, fo, mode)
    assert rep['faces_removed'] > 0 and rep['faces_out'] == len(sf) - rep['faces_removed']


def test_manifold_command_line(tmp_path):
    from points2surf_amd import manifold, ply
    indir, out, out2 = tmp_path / 'in', tmp_path / 'out', tmp_path / 'out2'
    indir.mkdir()
    clean, dirty = CASES['tetra'], CASES['tetras_sharing_an_edge']
    ply.write_ply(str(indir / 'clean.ply'), *clean)
    ply.write_ply(str(indir / 'dirty.ply'), *dirty)
    (indir / 'broken.ply').write_text('ply\nnot a mesh\n')
    assert manifold.main(['--indir', str(indir), '--outdir', str(out)]) == 0
    with open(out / 'manifold_report.csv', newline='') as fh:
        rows = {r['mesh']: r for r in csv.DictReader(fh)}
    assert list(rows['clean.ply']) == list(manifold.REPORT_COLUMNS) and sorted(rows) == ['broken.ply', 'clean.ply', 'dirty.ply']
    assert rows['broken.ply']['verdict'].startswith('failed: ') and not os.path.exists(out / 'broken.ply')
    c, d = rows['clean.ply'], rows['dirty.ply']
    assert (c['edges'], c['verts_in'], c['verts_out'], c['faces_out'], c['nonmanifold_edges_in'], c['vertices_added'], c['verdict']) == \
        ('split', '4', '4', '4', '0', '0', 'closed')
    m = MM.manifold(*dirty, 2)
    assert (d['verts_in'], d['verts_out'], d['faces_out'], d['nonmanifold_edges_in'], d['faces_removed'], d['vertices_split'], d['vertices_added'],
            d['rejoined_edges'], d['boundary_edges_out'], d['holes_filled'], d['watertight'], d['verdict']) == \
        ('8', '8', '8', '1', '0', '2', '2', '2', '0', '', '', 'closed')                 # 6 of the 8 input vertices are referenced
    gv, gf = ply.read_ply(str(out / 'dirty.ply'))
    assert np.asarray(gv, np.float32).tobytes() == m['verts'].tobytes() and np.array_equal(np.asarray(gf).reshape(-1, 3), m['faces'])
    gv, gf = ply.read_ply(str(out / 'clean.ply'))
    assert np.asarray(gv, np.float32).tobytes() == clean[0].tobytes() and np.array_equal(np.asarray(gf).reshape(-1, 3), clean[1])
    # a second run: both up to date, the rows kept; the broken one is tried again
    stamp = os.path.getmtime(out / 'dirty.ply')
    os.utime(indir / 'clean.ply', (1, 1))
    os.utime(indir / 'dirty.ply', (1, 1))
    assert manifold.manifold_dir(str(indir), str(out)) == []
    assert os.path.getmtime(out / 'dirty.ply') == stamp
    with open(out / 'manifold_report.csv', newline='') as fh:
        assert {r['mesh']: r for r in csv.DictReader(fh)} == rows
    # the other sequence on the same directory is not up to date: other rows
    assert sorted(os.path.basename(p) for p in manifold.manifold_dir(str(indir), str(out), edges='remove')) == ['clean.ply', 'dirty.ply']
    # --edges remove with --dataset: mode 1, the repair with its hole filling, mode 2
    (tmp_path / 'set.txt').write_text('dirty\n')
    assert manifold.main(['--indir', str(indir), '--outdir', str(out2), '--edges', 'remove', '--max_hole_edges', '30',
                          '--dataset', str(tmp_path / 'set.txt')]) == 0
    assert sorted(os.listdir(out2)) == ['dirty.ply', 'manifold_report.csv']
    with open(out2 / 'manifold_report.csv', newline='') as fh:
        rows2 = list(csv.DictReader(fh))
    first = MM.manifold(*dirty, 1)
    r = rows2[0]
    assert len(rows2) == 1 and (r['edges'], r['verts_in'], r['faces_in'], r['nonmanifold_edges_in'], r['faces_removed']) == \
        ('remove', '8', '8', '1', str(first['report'][4]))
    assert r['holes_filled'] != '' and r['watertight'] in ('0', '1') and r['verdict'] in ('closed', 'open')
    gv, gf = ply.read_ply(str(out2 / 'dirty.ply'))
    assert MM.defects(np.asarray(gf).reshape(-1, 3)) == (0, 0) and len(gf) == int(r['faces_out']) and len(gv) == int(r['verts_out'])
