"""The reconstruction-quality report on the device (metrics.mesh_quality, quality_comparison, the command line) and its
reductions (p2s_surface_stats, p2s_occupancy_counts) against numpy on the device's own per-sample arrays
(tests/quality_model.py), on a mesh against itself and on two concentric cubes."""
import os

import numpy as np
import pytest
import torch

import quality_model as Q
import voxel_model as V
from test_mesh_sdf_model import GOLDEN, MESHES, load

pytestmark = pytest.mark.gpu

DELTA = 1.0 / 64.0
OUTER = np.float32(0.3)
INNER = np.float32(OUTER - np.float32(DELTA))


def _trimesh(v, f):
    from points2surf_amd import gt_sdf
    return gt_sdf.TriMesh(np.asarray(v, np.float32), np.asarray(f, np.int32))


def _samples(v, f, n, seed):
    """n area-weighted samples of the mesh and their faces, on the device"""
    from points2surf_amd import engine, metrics
    vt, ft = torch.from_numpy(np.asarray(v, np.float32)).cuda(), torch.from_numpy(np.asarray(f, np.int32)).cuda()
    pts, _, fid = metrics.sample_surface(vt, ft, n, engine.Rng(seed), want_faces=True)
    return pts, fid


def _write(path, v, f):
    from points2surf_amd import ply
    ply.write_ply(path, np.asarray(v, np.float32), np.asarray(f, np.int32))


@pytest.mark.parametrize('n', [1, 4099, 70001])
def test_reductions_against_numpy_on_the_device_arrays(n):
    """counts exact; sums within 2 n 2^-53 relative (non-negative terms: the bound of any order of summation); the mean
    normal term within 2^-44 (the model's unit normals differ from the stored ones by a few 2^-53); two runs, the same bits.
    n = 70001 makes threads add a second term (the grid has 65536)."""
    from points2surf_amd import metrics
    (va, fa), (vb, fb) = load(MESHES[2])[:2], load(MESHES[1])[:2]
    a, b = _trimesh(va, fa), _trimesh(vb, fb)
    try:
        pts, fid = _samples(va, fa, n, 7)
        d, face_to = b.distance(pts, signed=False, want_face=True)
        taus = (0.005, 0.01, 0.05, float(d.median()))
        got = metrics.surface_stats(a, b, d, fid, face_to, taus)
        again = metrics.surface_stats(a, b, d, fid, face_to, taus)
    finally:
        a.close()
        b.close()
    assert got == again
    want = Q.surface_stats(d.cpu().numpy(), fid.cpu().numpy(), face_to.cpu().numpy(), Q.unit_normals(va, fa), Q.unit_normals(vb, fb), taus)
    print(n, got, want)
    assert got['counts'] == want['counts'] and 0 < got['nc_pairs'] == want['nc_pairs'] <= n and got['max'] == want['max']
    rel = 2.0 * n * 2.0 ** -53
    assert abs(got['sum'] - want['sum']) <= rel * want['sum'] and abs(got['sum_sq'] - want['sum_sq']) <= rel * want['sum_sq']
    assert abs(got['sum_nc'] - want['sum_nc']) / got['nc_pairs'] <= 2.0 ** -44
    assert want['counts'][3] >= (n + 1) // 2                  # the median itself counts: d <= tau


def test_reductions_leave_out_degenerate_faces_and_take_no_threshold():
    from points2surf_amd import metrics
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3]], np.int32)            # the second face has no area: its stored normal is 0
    m = _trimesh(v, f)
    try:
        d = torch.tensor([0.5, 0.25, 2.0], dtype=torch.float64, device='cuda')
        ff = torch.tensor([0, 1, 0], dtype=torch.int32, device='cuda')
        ft = torch.tensor([0, 0, -1], dtype=torch.int32, device='cuda')
        got = metrics.surface_stats(m, m, d, ff, ft, ())
    finally:
        m.close()
    assert got == dict(sum=2.75, sum_sq=0.25 + 0.0625 + 4.0, max=2.0, sum_nc=1.0, nc_pairs=1, counts=[])


@pytest.mark.parametrize('n', [1, 7, 8, 4097, 32 ** 3])
def test_occupancy_counts(n):
    from points2surf_amd import metrics
    rs = np.random.RandomState(n)
    a, b = (rs.randint(0, 2, n).astype(np.uint8) for _ in range(2))
    assert metrics.occupancy_counts(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) == Q.occupancy_counts(a, b)


def test_cube_against_itself(tmp_path):
    """half-side 0.25: a sample of an axis face keeps the face's coordinate exactly, so it lies ON the surface; the distance
    kernel rebuilds the closest point as a + v ab + w ac in float64, a few units of 2^-53 of the coordinate magnitude 0.25
    per axis: every distance is 0 to within 2^-50"""
    from points2surf_amd import metrics
    path = str(tmp_path / 'cube.ply')
    _write(path, *V.cube(0.25))
    q = metrics.mesh_quality(path, path, samples_per_model=4096, iou_res=16)
    print(q)
    assert 0.0 <= q['accuracy_max'] <= 2.0 ** -50 and 0.0 <= q['completeness_max'] <= 2.0 ** -50
    assert q['hausdorff'] == max(q['accuracy_max'], q['completeness_max']) and 0.0 <= q['chamfer_l1'] <= 2.0 ** -50
    assert q['fscore@0.005'] == 1.0 and q['fscore@0.01'] == 1.0
    assert abs(q['normal_consistency'] - 1.0) <= 2.0 ** -44
    assert q['iou'] == 1.0 and q['note'] == '' and q['samples'] == 4096 and q['iou_res'] == 16


def test_fixture_mesh_against_itself():
    """the samples are float32 roundings of points of the surface: within a few 2^-24 of it, far below 1e-6"""
    from points2surf_amd import metrics
    path = os.path.join(GOLDEN, '03_meshes', MESHES[2])
    q = metrics.mesh_quality(path, path, samples_per_model=4096, iou_res=32)
    print(q)
    assert 0.0 <= q['hausdorff'] < 1e-6 and q['fscore@0.005'] == 1.0 and q['fscore@0.01'] == 1.0
    assert q['normal_consistency'] > 0.99 and q['iou'] == 1.0


def test_concentric_cubes(tmp_path):
    """new = the inner cube (half-side 0.3 - delta), ref = the outer one (0.3), delta = 1/64, 4096 samples each.  Every inner
    sample lies delta from the outer surface.  The outer samples are 4088 drawn ones and the 8 corners, which lie
    delta sqrt(3) from the inner cube (drawn samples alone come only near a corner).  IoU at R = 16 from the exact model."""
    from points2surf_amd import metrics
    (vi, fi), (vo, fo) = V.cube(INNER), V.cube(OUTER)
    inner, outer = _trimesh(vi, fi), _trimesh(vo, fo)
    taus = (1.001 * DELTA, 0.999 * DELTA)
    try:
        pts, fid = _samples(vi, fi, 4096, 3)
        d, face_to = outer.distance(pts, signed=False, want_face=True)
        acc = metrics.surface_stats(inner, outer, d, fid, face_to, taus)
        pts, fid = _samples(vo, fo, 4088, 4)
        corner_face = np.array([[k for k in range(12) if c in fo[k]][0] for c in range(8)], np.int32)
        pts = torch.cat([pts, torch.from_numpy(vo).cuda()])
        fid = torch.cat([fid, torch.from_numpy(corner_face).cuda()])
        d, face_to = inner.distance(pts, signed=False, want_face=True)
        com = metrics.surface_stats(outer, inner, d, fid, face_to, taus)
        counts = metrics.occupancy_counts(inner.voxelize(16), outer.voxelize(16))
    finally:
        inner.close()
        outer.close()
    print(acc, com, counts)
    assert abs(acc['sum'] / 4096 - DELTA) < 1e-6 and abs(acc['max'] - DELTA) < 1e-6
    assert acc['counts'] == [4096, 0]                          # precision 1 at 1.001 delta, 0 at 0.999 delta
    assert abs(com['max'] - DELTA * np.sqrt(3.0)) < 1e-6
    assert np.abs(d.cpu().numpy()[-8:] - Q.box_distance(vo, INNER)).max() < 1e-12      # the corners themselves
    occ = [V.exact(*V.cube(h), 16)[0] != 0 for h in (INNER, OUTER)]
    assert counts == Q.occupancy_counts(*occ) == (64, 64, 64)
    path_i, path_o = str(tmp_path / 'inner.ply'), str(tmp_path / 'outer.ply')
    _write(path_i, vi, fi)
    _write(path_o, vo, fo)
    q = metrics.mesh_quality(path_i, path_o, samples_per_model=4096, taus=taus, iou_res=16)
    print(q)
    assert abs(q['accuracy_mean'] - DELTA) < 1e-6 and q['precision@%g' % taus[0]] == 1.0 and q['precision@%g' % taus[1]] == 0.0
    assert q['iou'] == Q.iou(*occ) == 1.0 and DELTA - 1e-6 < q['completeness_max'] < DELTA * np.sqrt(3.0) + 1e-6
    assert q['normal_consistency'] > 0.9


def _directory(tmp_path):
    """new/ and ref/ without a data set file (the reference then compares file names WITHOUT an extension): `pair` and
    `open` are compared; `extra.ply` lies outside the set to compare and has a reference: -2, and, as the reference has
    it, its reference counts as never reconstructed: -1, like `lonely`"""
    new_dir, ref_dir = str(tmp_path / 'new'), str(tmp_path / 'ref')
    os.makedirs(new_dir)
    os.makedirs(ref_dir)
    _write(os.path.join(new_dir, 'pair'), *V.cube(INNER))
    _write(os.path.join(ref_dir, 'pair'), *V.cube(OUTER))
    _write(os.path.join(new_dir, 'open'), *V.open_cube(INNER))
    _write(os.path.join(ref_dir, 'open'), *V.cube(OUTER))
    _write(os.path.join(new_dir, 'extra.ply'), *V.cube(INNER))
    _write(os.path.join(ref_dir, 'extra.ply'), *V.cube(OUTER))
    _write(os.path.join(ref_dir, 'lonely'), *V.cube(OUTER))
    return new_dir, ref_dir


def test_csv_and_command_line(tmp_path, capsys):
    from points2surf_amd import metrics
    new_dir, ref_dir = _directory(tmp_path)
    report = str(tmp_path / 'out' / 'quality.csv')
    kw = dict(samples_per_model=2048, taus=(0.02,), iou_res=16, seed=5)
    rows = metrics.quality_comparison(new_dir, ref_dir, report, **kw)
    lines = open(report).read().split('\n')
    keys = metrics.quality_keys((0.02,))
    head = lines[0].split(',')
    assert head[:2] == ['in mesh', 'ref mesh'] and head[2:-1] == keys[:-1] and head[-1].startswith('iou_res')
    assert len(lines) == 1 + 5 and len(rows) == 5 and all(len(l.split(',')) == len(head) for l in lines)
    by = dict((os.path.basename(l.split(',')[0]) + ':' + l.split(',')[2], dict(zip(keys, l.split(',')[2:]))) for l in lines[1:])
    pair = [v for k, v in by.items() if k.startswith('pair:')][0]
    direct = metrics.mesh_quality(os.path.join(new_dir, 'pair'), os.path.join(ref_dir, 'pair'), **kw)
    assert pair == dict((k, direct[k] if k == 'note' else repr(direct[k])) for k in keys)
    assert float(pair['iou']) == 1.0 and pair['note'] == '' and pair['samples'] == '2048' and pair['iou_res'] == '16'
    # every inner sample lies delta = 0.0156 from the outer surface; an outer sample within 0.0031 of an edge of its face
    # lies more than 0.02 from the inner cube (delta^2 + e^2 > 0.02^2 for e > 0.0125): about 2 % of the area
    p, r = float(pair['precision@0.02']), float(pair['recall@0.02'])
    assert abs(float(pair['accuracy_mean']) - DELTA) < 1e-6 and p == 1.0 and 0.95 < r < 1.0
    assert float(pair['fscore@0.02']) == 2.0 * p * r / (p + r)
    opened = [v for k, v in by.items() if k.startswith('open:')][0]
    assert opened['iou'] == '-1.0' and opened['note'] == 'new mesh not closed' and abs(float(opened['accuracy_mean']) - DELTA) < 1e-6
    assert float(opened['hausdorff']) > 0.0 and float(opened['normal_consistency']) > 0.9
    assert by['extra.ply:-2']['iou'] == '-2' and by['extra.ply:-2']['note'] == 'no reference'
    assert by['extra.ply:-1']['hausdorff'] == '-1' and by['lonely:-1']['note'] == 'no input' and by['lonely:-1']['samples'] == '2048'
    # the command line writes the same file
    cli = str(tmp_path / 'cli.csv')
    metrics.main(['--new', new_dir, '--ref', ref_dir, '--report', cli, '--samples', '2048', '--tau', '0.02', '--iou_res', '16',
                  '--seed', '5'])
    assert open(cli).read() == open(report).read()
    assert capsys.readouterr().out.count('\n') == 5
    # a malformed mesh: the -1 convention, with its note
    bad = str(tmp_path / 'bad')
    open(bad, 'w').write('ply\nnot a mesh')
    q = metrics.mesh_quality(bad, os.path.join(ref_dir, 'pair'), **kw)
    assert q['hausdorff'] == -1.0 and q['iou'] == -1.0 and q['note'] == 'no input'


def test_mesh_comparison_writes_what_it_wrote(tmp_path):
    """the pairing moved into a function of its own: mesh_comparison's file on the same directory is, byte for byte, the
    header and the rows its earlier body put together"""
    from points2surf_amd import metrics
    new_dir, ref_dir = _directory(tmp_path)
    report = str(tmp_path / 'hausdorff.csv')
    metrics.mesh_comparison(new_dir, ref_dir, 3, report, samples_per_model=500, seed=2)
    rows = []
    for name in ('open', 'pair'):
        a, b = os.path.join(new_dir, name), os.path.join(ref_dir, name)
        rows.append((a, b) + tuple(str(x) for x in metrics.mesh_distances(a, b, 500, seed=2)))
    a, b = os.path.join(new_dir, 'extra.ply'), os.path.join(ref_dir, 'extra.ply')
    rows += [(a, b, '-2', '-2', '-2', '-2'), (a, b, '-1', '-1', '-1', '-1')]
    rows.append((os.path.join(new_dir, 'lonely'), os.path.join(ref_dir, 'lonely'), '-1', '-1', '-1', '-1'))
    want = ['in mesh,ref mesh,Hausdorff dist new-ref,Hausdorff dist ref-new,Hausdorff dist,Chamfer dist(-1: no input; -2: no reference)']
    want += [','.join(r) for r in sorted(rows, key=lambda x: x[0])]
    assert open(report).read() == '\n'.join(want)
