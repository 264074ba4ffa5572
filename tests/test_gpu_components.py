"""Components of meshes and clusters of clouds on the device (p2s_mesh_components, p2s_mesh_submesh, p2s_prepare_clusters;
points2surf_amd/components.py, prepare.remove_small_clusters) against the numpy model (tests/components_model.py): labels,
ranks, integer counts, boxes, kept ids and sub-mesh arrays for EQUALITY; areas and volumes within the forward bound of any
float64 summation order, |got - fsum| <= (faces + 8) 2^-52 sum |term| (the per-face terms are bit-equal to numpy's by
construction); determinism; the capacity conventions; prepare and the two command lines on temporary directories.

"The partners just outside: 27 clusters" cannot be one cloud -- 26 points on a sphere of the radius are never pairwise further
apart than the radius -- so it is one cloud per partner (two clusters each), and the cloud of all of them against the model
with the centre alone in its cluster."""
import csv
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

import components_model as CM
import prepare_model as PM

pytestmark = pytest.mark.gpu

P2S_EINVAL = -1
PAD = 1024
MESHES = CM.small_cases()
CLOUDS = CM.cluster_cases()


@functools.lru_cache(maxsize=None)
def big():
    v, f = CM.big_case()
    return v, f, CM.mesh_components(v, f)


def _dev():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def raw_components(v, f, cap=None):
    """the raw call with every output filled with a pattern first and PAD entries of it behind -> rc, numpy arrays, report"""
    import torch
    from points2surf_amd import _lib, engine
    lib, dev = _lib.load(), _dev()
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    V, F = len(v), len(f)
    cap = F if cap is None else cap
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    comp = torch.full((F + PAD,), -77, dtype=torch.int32, device=dev)
    counts = torch.full((5 * cap + PAD,), -77, dtype=torch.int64, device=dev)
    meas = torch.full((8 * cap + PAD,), -77.0, dtype=torch.float64, device=dev)
    rep = (ctypes.c_int64 * 8)(*([-1] * 8))
    ptr = lambda t, n: engine._ptr(t) if n else None
    rc = lib.p2s_mesh_components(ptr(tv, V), V, ptr(tf, F), F, engine._ptr(comp), cap, engine._ptr(counts), engine._ptr(meas), rep,
                                 dev.index, engine._stream_ptr(dev))
    return rc, comp.cpu().numpy(), counts.cpu().numpy(), meas.cpu().numpy(), np.array(rep[:], np.int64)


def check_components(v, f, m, got):
    rc, comp, counts, meas, rep = got
    F, C = len(f), int(m['report'][1])
    assert rc == 0
    assert rep[:5].tolist() == m['report'][:5].tolist() and rep[6:].tolist() == [0, 0]
    assert np.array_equal(comp[:F], m['comp']) and np.all(comp[F:] == -77)
    assert np.array_equal(counts[:5 * C].reshape(C, 5), m['counts']) and np.all(counts[5 * C:] == -77)
    q = meas[:8 * C].reshape(C, 8)
    assert np.all(meas[8 * C:] == -77.0)
    assert np.array_equal(q[:, 2:], m['measures'][:, 2:])
    bound = (m['counts'][:, 1] + 8) * 2.0 ** -52
    err_a, err_v = np.abs(q[:, 0] - m['measures'][:, 0]), np.abs(q[:, 1] - m['measures'][:, 1])
    print('area: max error %.3g of bound %.3g; volume: %.3g of %.3g' % (err_a.max(initial=0), (bound * m['abs_area']).max(initial=0),
                                                                        err_v.max(initial=0), (bound * m['abs_volume']).max(initial=0)))
    assert np.all(err_a <= bound * m['abs_area']) and np.all(err_v <= bound * m['abs_volume'])


@pytest.mark.parametrize('name', sorted(MESHES))
def test_small_meshes(name):
    v, f = MESHES[name]
    check_components(v, f, CM.mesh_components(v, f), raw_components(v, f))


def test_single_term_components_are_numpy_bits():
    """a component of one face holds that face's terms: the float64 expressions are numpy's, bit for bit"""
    rng = np.random.RandomState(4)
    v = rng.normal(size=(3 * 300, 3)).astype(np.float32)
    f = np.arange(900, dtype=np.int32).reshape(-1, 3)
    rc, _, _, meas, _ = raw_components(v, f)
    area, vol = CM.face_terms(v, f)
    q = meas[:8 * 300].reshape(300, 8)
    assert rc == 0 and np.array_equal(q[:, 0], area) and np.array_equal(q[:, 1], vol)


def test_more_components_than_the_first_capacity():
    """70,000 separate triangles: the raw call refuses 65,536 with the report filled and nothing written; the Python call
    repeats with the exact count; ranks equal face ids"""
    from points2surf_amd import components
    v, f = CM.separate_triangles(70000)
    rc, comp, counts, meas, rep = raw_components(v, f, cap=65536)
    assert rc == P2S_EINVAL and rep[:5].tolist() == [len(v) | (70000 << 32), 70000, 1, 0, 0]
    assert np.all(comp == -77) and np.all(counts == -77) and np.all(meas == -77.0)
    comp, st, r = components.components(v, f)
    assert r['components'] == 70000 and np.array_equal(comp.cpu().numpy(), np.arange(70000))
    assert np.array_equal(st['first_face'], np.arange(70000)) and np.all(st['faces'] == 1) and np.all(st['boundary_edges'] == 3)
    assert np.array_equal(st['area'], CM.face_terms(v, f)[0]) and not st['closed'].any()


def test_cavity_and_quad_and_fan_through_python():
    from points2surf_amd import components
    v, f = MESHES['tetra_with_cavity']
    comp, st, r = components.components(v, f)
    assert r['components'] == 2 and st['closed'].tolist() == [True, True] and st['volume'][0] > 0 > st['volume'][1]
    vo, fo, rep = components.filter_mesh(v, f)
    assert rep['cavities'] == 1 and rep['closed_components'] == 2 and rep['components_kept'] == 2           # 1/16 of the area stays
    vo, fo, rep = components.filter_mesh(v, f, min_area_share=0.1)
    assert rep['components_kept'] == 1 and rep['faces_out'] == 4 and np.array_equal(vo.cpu().numpy(), v[:4])
    assert abs(rep['largest_removed_area_share'] - 1.0 / 17.0) < 1e-12
    assert components.components(*MESHES['quad'])[1]['boundary_edges'].tolist() == [4]
    assert components.components(*MESHES['three_faces_on_one_edge'])[1]['nonmanifold_edges'].tolist() == [1]


def test_big_case_and_determinism():
    v, f, m = big()
    assert m['report'][1] == 41 and m['report'][2] == 300000
    a = raw_components(v, f)
    check_components(v, f, m, a)
    b = raw_components(v, f)
    for x, y in zip(a[1:4], b[1:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4][:5].tolist() == b[4][:5].tolist()


def test_invalid_meshes_are_refused():
    v, f = MESHES['quad']
    bad = f.copy()
    bad[1, 2] = 4
    assert raw_components(v, bad)[0] == P2S_EINVAL
    bad[1, 2] = -1
    assert raw_components(v, bad)[0] == P2S_EINVAL
    nan = v.copy()
    nan[2, 1] = np.nan
    assert raw_components(nan, f)[0] == P2S_EINVAL


# ---- the sub-mesh ----------------------------------------------------------------------------------------------------------

def raw_submesh(v, f, keep, cap_verts=None, cap_faces=None):
    import torch
    from points2surf_amd import _lib, engine
    lib, dev = _lib.load(), _dev()
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    V, F = len(v), len(f)
    cv, cf = V if cap_verts is None else cap_verts, F if cap_faces is None else cap_faces
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    tk = torch.from_numpy(np.ascontiguousarray(keep, np.int32)).to(dev)
    vo = torch.full((3 * cv + PAD,), 77.0, dtype=torch.float32, device=dev)
    fo = torch.full((3 * cf + PAD,), -77, dtype=torch.int32, device=dev)
    so = torch.full((cf + PAD,), -77, dtype=torch.int32, device=dev)
    mo = torch.full((V + PAD,), -77, dtype=torch.int32, device=dev)
    rep = (ctypes.c_int64 * 3)()
    rc = lib.p2s_mesh_submesh(engine._ptr(tv), V, engine._ptr(tf), F, engine._ptr(tk), engine._ptr(vo), cv, engine._ptr(fo), engine._ptr(so),
                              cf, engine._ptr(mo), rep, dev.index, engine._stream_ptr(dev))
    return rc, vo.cpu().numpy(), fo.cpu().numpy(), so.cpu().numpy(), mo.cpu().numpy(), [int(x) for x in rep]


def check_submesh(v, f, keep):
    wv, wf, wsrc, wmap = CM.submesh(v, f, keep)
    rc, vo, fo, so, mo, rep = raw_submesh(v, f, keep)
    nv, nf = len(wv), len(wf)
    assert rc == 0 and rep == [len(v) | (len(f) << 32), nv, nf]
    assert vo[:3 * nv].tobytes() == wv.tobytes() and np.all(vo[3 * nv:] == 77.0)
    assert np.array_equal(fo[:3 * nf].reshape(-1, 3), wf) and np.all(fo[3 * nf:] == -77)
    assert np.array_equal(so[:nf], wsrc) and np.all(so[nf:] == -77)
    assert np.array_equal(mo[:len(v)], wmap) and np.all(mo[len(v):] == -77)


def test_every_mask_of_a_six_face_mesh():
    v, f = CM.join([CM.tetra(1.0), MESHES['shared_vertex']], seed=2)
    assert len(f) == 6
    for mask in itertools.product((0, 1), repeat=6):
        check_submesh(v, f, np.array(mask) * 5)               # nonzero = keep


def test_submesh_of_the_big_case_and_the_capacity_refusal():
    from points2surf_amd import components
    v, f, m = big()
    keep = CM.select(CM.stats(m), min_area_share=0.0001)
    assert 1 <= keep.sum() < 41
    mask = keep[m['comp']].astype(np.int32)
    check_submesh(v, f, mask)
    check_submesh(v, f, np.zeros(len(f), np.int32))
    wv, wf, _, _ = CM.submesh(v, f, mask)
    vo, fo, rep = components.filter_mesh(v, f, min_area_share=0.0001)
    assert vo.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(fo.cpu().numpy(), wf)
    assert rep['components'] == 41 and rep['components_kept'] == int(keep.sum()) and rep['keep'].tolist() == keep.tolist()
    for cv, cf in ((len(wv) - 1, len(wf)), (len(wv), len(wf) - 1)):
        rc, vo, fo, so, mo, r = raw_submesh(v, f, mask, cap_verts=cv, cap_faces=cf)
        assert rc == P2S_EINVAL and r[1:] == [len(wv), len(wf)]
        assert np.all(vo == 77.0) and np.all(fo == -77) and np.all(so == -77) and np.all(mo == -77)


# ---- clusters --------------------------------------------------------------------------------------------------------------

def raw_clusters(p, radius, min_points):
    import torch
    from points2surf_amd import _lib, engine
    lib, dev = _lib.load(), _dev()
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    n = len(p)
    tp = torch.from_numpy(p).to(dev) if n else torch.zeros((1, 3), dtype=torch.float32, device=dev)
    lab = torch.full((n + PAD,), -77, dtype=torch.int32, device=dev)
    out = torch.full((3 * n + PAD,), 77.0, dtype=torch.float32, device=dev)
    ids = torch.full((n + PAD,), -77, dtype=torch.int32, device=dev)
    m, info = ctypes.c_int64(-1), (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    rc = lib.p2s_prepare_clusters(engine._ptr(tp), n, ctypes.c_double(radius), min_points, engine._ptr(lab), engine._ptr(out), engine._ptr(ids),
                                  ctypes.byref(m), info, dev.index, engine._stream_ptr(dev))
    return rc, lab.cpu().numpy(), out.cpu().numpy(), ids.cpu().numpy(), m.value, [int(x) for x in info]


def check_clusters(p, radius, min_points):
    want = CM.clusters(p, radius, min_points)
    rc, lab, out, ids, m, info = raw_clusters(p, radius, min_points)
    n, k = len(p), len(want['ids'])
    assert rc == 0 and m == k and info == want['info'].tolist()
    assert np.array_equal(lab[:n], want['labels']) and np.all(lab[n:] == -77)
    assert np.array_equal(ids[:k], want['ids']) and np.all(ids[k:] == -77)
    assert out[:3 * k].tobytes() == want['points'].tobytes() and np.all(out[3 * k:] == 77.0)
    return want


@pytest.mark.parametrize('name', sorted(CLOUDS))
def test_clusters(name):
    p, radius = CLOUDS[name]
    want = check_clusters(p, radius, 1)
    if name == 'lattice70000':
        assert np.array_equal(want['labels'], np.arange(70000))
    if name == 'star_outside':
        assert (want['labels'] == 0).sum() == 1
        for k in range(1, 27):
            assert check_clusters(p[[0, k]], radius, 1)['info'][:2].tolist() == [2, 1]


@pytest.mark.parametrize('min_points', [1, 6, 51, 301, 10 ** 6])
def test_small_clusters_are_removed(min_points):
    p, radius = CLOUDS['clumps']
    want = check_clusters(p, radius, min_points)
    assert want['info'][3] == {1: 0, 6: 1, 51: 2, 301: 3, 10 ** 6: 3}[min_points]


def test_cluster_refusals_on_the_device():
    from points2surf_amd import _lib
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 3e6, 0]], np.float32)
    assert raw_clusters(p, 1.0, 1)[0] == P2S_EINVAL and b'radius too small for this extent' in _lib.load().p2s_last_error()
    assert raw_clusters(p, 3.0, 1)[0] == 0                                                                 # 10^6 cells: fine
    p[1, 2] = np.inf
    assert raw_clusters(p, 1e6, 1)[0] == P2S_EINVAL


# ---- prepare and the command lines -----------------------------------------------------------------------------------------

def test_prepare_with_the_cluster_stage():
    from points2surf_amd import prepare
    p, radius = CLOUDS['clumps']
    want = CM.clusters(p, radius, 60)
    assert want['info'][3] == 2 and len(want['ids']) == 20300
    pts, kept, frame, rep = prepare.prepare(p, crop_quantile=0.0, std_ratio=0.0, max_points=0, min_cluster=60, cluster_radius=radius)
    assert np.array_equal(frame['kept'].cpu().numpy(), want['ids']) and np.array_equal(kept.cpu().numpy(), want['ids'])
    assert pts.cpu().numpy().tobytes() == PM.normalize(want['points'])[0].tobytes()
    assert (rep['clusters'], rep['small_clusters'], rep['cluster_points'], rep['cluster_radius']) == (4, 2, 55, radius)
    # the automatic radius: cluster_factor times the outlier stage's mean, on what that stage left
    o_pts, o_ids, info = prepare.remove_outliers(p, 16, 2.0, want_report=True)
    auto = CM.clusters(o_pts.cpu().numpy(), 3.0 * info['mean'], 60)
    pts, kept, frame, rep = prepare.prepare(p, crop_quantile=0.0, max_points=0, min_cluster=60)
    assert rep['cluster_radius'] == 3.0 * info['mean'] and rep['clusters'] == auto['info'][0] and rep['small_clusters'] == auto['info'][3]
    assert np.array_equal(kept.cpu().numpy(), o_ids.cpu().numpy()[auto['ids']])
    # off: what it was
    a = prepare.prepare(p, crop_quantile=0.0, max_points=0)
    assert sorted(a[3]) == sorted(['points_in', 'nonfinite', 'cropped', 'outliers', 'thinned', 'points_out', 'R', 'mean', 'std', 'threshold'])
    assert np.array_equal(a[1].cpu().numpy(), o_ids.cpu().numpy())


def test_prepare_command_line(tmp_path):
    from points2surf_amd import prepare
    p, radius = CLOUDS['clumps']
    raw, off, on = tmp_path / 'raw', tmp_path / 'off', tmp_path / 'on'
    raw.mkdir()
    np.save(raw / 'scan.npy', p)
    common = ['--indir', str(raw), '--crop_quantile', '0', '--std_ratio', '0', '--max_points', '0']
    assert prepare.main(common + ['--outdir', str(off)]) == 0
    assert not os.path.exists(off / 'clusters_report.csv')
    assert prepare.main(common + ['--outdir', str(on), '--min_cluster', '60', '--cluster_radius', repr(radius)]) == 0
    with open(on / 'clusters_report.csv', newline='') as fh:
        rows = list(csv.DictReader(fh))
    assert rows == [dict(file='scan.npy', clusters='4', removed_clusters='2', removed_points='55', radius=repr(radius))]
    want = CM.clusters(p, radius, 60)
    assert np.load(on / '04_pts' / 'scan.xyz.npy').tobytes() == PM.normalize(want['points'])[0].tobytes()
    with open(off / 'prepare_report.csv', newline='') as fh:
        header = next(csv.reader(fh))
    with open(on / 'prepare_report.csv', newline='') as fh:
        assert next(csv.reader(fh)) == header == list(prepare.REPORT_COLUMNS)
    assert np.load(off / '04_pts' / 'scan.xyz.npy').tobytes() == PM.normalize(p)[0].tobytes()


def test_components_command_line(tmp_path):
    from points2surf_amd import components, ply
    indir, out, out2 = tmp_path / 'in', tmp_path / 'out', tmp_path / 'out2'
    indir.mkdir()
    clean = CM.torus(40, 20)
    dirty = CM.join([CM.torus(40, 20), CM.torus(3, 4, R=0.01, r=0.004, centre=(0.8, 0.8, 0.8)), CM.tetra(0.2, inward=True)], seed=1)
    ply.write_ply(str(indir / 'clean.ply'), *clean)
    ply.write_ply(str(indir / 'dirty.ply'), *dirty)
    argv = ['--indir', str(indir), '--outdir', str(out)]
    assert components.main(argv + ['--min_area_share', '0.001']) == 0
    with open(out / 'components_report.csv', newline='') as fh:
        rows = {r['mesh']: r for r in csv.DictReader(fh)}
    assert list(rows['clean.ply']) == list(components.REPORT_COLUMNS)
    c, d = rows['clean.ply'], rows['dirty.ply']
    assert (c['components'], c['components_kept'], c['faces_in'], c['faces_out'], c['verts_in'], c['verts_out']) == ('1', '1', '1600', '1600', '800', '800')
    assert (c['closed_components'], c['cavities'], c['verdict']) == ('1', '0', 'written') and float(c['largest_removed_area_share']) == 0.0
    m = CM.mesh_components(*dirty)
    keep = CM.select(CM.stats(m), min_area_share=0.001)
    assert keep.sum() == 2                                                              # the 24-face blob goes, the cavity stays
    wv, wf, _, _ = CM.submesh(*dirty, keep[m['comp']])
    assert (d['components'], d['components_kept'], d['faces_in'], d['faces_out'], d['verts_out']) == ('3', '2', '1628', '1604', str(len(wv)))
    assert (d['closed_components'], d['cavities']) == ('3', '1') and float(d['area_out']) < float(d['area_in'])
    gv, gf = ply.read_ply(str(out / 'dirty.ply'))
    assert np.asarray(gv, np.float32).tobytes() == wv.tobytes() and np.array_equal(np.asarray(gf).reshape(-1, 3), wf)
    gv, gf = ply.read_ply(str(out / 'clean.ply'))
    assert np.asarray(gv, np.float32).tobytes() == clean[0].tobytes() and np.array_equal(np.asarray(gf).reshape(-1, 3), clean[1])
    # a second run: both up to date, the rows kept
    stamp = os.path.getmtime(out / 'dirty.ply')
    os.utime(indir / 'clean.ply', (1, 1))
    os.utime(indir / 'dirty.ply', (1, 1))
    assert components.filter_dir(str(indir), str(out), min_area_share=0.001) == []
    assert os.path.getmtime(out / 'dirty.ply') == stamp
    with open(out / 'components_report.csv', newline='') as fh:
        assert {r['mesh']: r for r in csv.DictReader(fh)} == rows
    # --dataset
    (tmp_path / 'set.txt').write_text('dirty\n')
    assert components.main(['--indir', str(indir), '--outdir', str(out2), '--dataset', str(tmp_path / 'set.txt'), '--max_components', '1']) == 0
    assert sorted(os.listdir(out2)) == ['components_report.csv', 'dirty.ply']
    with open(out2 / 'components_report.csv', newline='') as fh:
        rows2 = list(csv.DictReader(fh))
    assert len(rows2) == 1 and rows2[0]['components_kept'] == '1' and rows2[0]['faces_out'] == '1600'
