"""p2s_mesh_fill_holes on the device (points2surf_amd/holes.py) against the numpy model (tests/holes_model.py) for EQUALITY on
every case: faces, face_src, the per-hole table, the areas bit for bit, report [0..11]; nothing written beyond the counts;
determinism; idempotence; the capacity refusal; agreement with the existing, independent units (p2s_mesh_components counts the
same edges, p2s_mesh_check no new non-manifold vertex, p2s_mesh_voxelize accepts the closed result); the opt-in of
points2surf_amd.manifold; the command line."""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest

import holes_model as HM

pytestmark = pytest.mark.gpu

P2S_EINVAL = -1
PAD = 1024
SMALL = HM.small_cases()
LONG = HM.long_cases()


@functools.lru_cache(maxsize=None)
def many():
    v, f, K = HM.many_holes()
    return v, f, K, HM.fill(v, f, K)


def _dev():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def raw_fill(v, f, K, cap_faces=None, cap_holes=None, optional=True):
    """the raw call with every output filled with a pattern first and PAD entries of it behind -> rc, numpy arrays, report"""
    import torch
    from points2surf_amd import _lib, engine
    lib, dev = _lib.load(), _dev()
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    V, F = len(v), len(f)
    nb = len(HM.boundary(f))
    cf, ch = F + nb if cap_faces is None else cap_faces, nb // 3 if cap_holes is None else cap_holes
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    fo = torch.full((3 * cf + PAD,), -77, dtype=torch.int32, device=dev)
    fs = torch.full((cf + PAD,), -77, dtype=torch.int32, device=dev)
    ho = torch.full((4 * ch + PAD,), -77, dtype=torch.int32, device=dev)
    ha = torch.full((ch + PAD,), 77.0, dtype=torch.float64, device=dev)
    rep = (ctypes.c_int64 * 16)(*([-1] * 16))
    ptr = lambda t, n: engine._ptr(t) if n else None
    opt = lambda t: engine._ptr(t) if optional else None
    rc = lib.p2s_mesh_fill_holes(ptr(tv, V), V, ptr(tf, F), F, K, engine._ptr(fo), cf, opt(fs), opt(ho), opt(ha), ch, rep, dev.index,
                                 engine._stream_ptr(dev))
    return rc, fo.cpu().numpy(), fs.cpu().numpy(), ho.cpu().numpy(), ha.cpu().numpy(), np.array(rep[:], np.int64)


def check_fill(m, got, optional=True):
    rc, fo, fs, ho, ha, rep = got
    nf, nh = len(m['faces']), len(m['holes'])
    assert rc == 0
    assert rep[:12].tolist() == m['report'][:12].tolist() and rep[12:].tolist() == [0, 0, 0, 0]
    assert np.array_equal(fo[:3 * nf].reshape(-1, 3), m['faces']) and np.all(fo[3 * nf:] == -77)
    if optional:
        assert np.array_equal(fs[:nf], m['face_src']) and np.all(fs[nf:] == -77)
        assert np.array_equal(ho[:4 * nh].reshape(-1, 4), m['holes']) and np.all(ho[4 * nh:] == -77)
        assert ha[:nh].tobytes() == m['hole_area'].tobytes() and np.all(ha[nh:] == 77.0)
    else:
        assert np.all(fs == -77) and np.all(ho == -77) and np.all(ha == 77.0)


def check_independent(v, f, m):
    """the existing units on the output: the edges of more than two faces of the input, the boundary edges of report [8]
    (components); no non-manifold vertex that the input had not (mesh check)"""
    from points2surf_amd import components, gt_sdf
    if len(f) == 0:
        return
    before, after = components.components(v, f)[1], components.components(v, m['faces'])[1]
    assert int(after['nonmanifold_edges'].sum()) == int(before['nonmanifold_edges'].sum()) == m['report'][11]
    assert int(after['boundary_edges'].sum()) == m['report'][8]
    counts = []
    for faces in (f, m['faces']):
        mesh = gt_sdf.TriMesh(v, faces)
        try:
            counts.append(mesh.check()['nonmanifold_vertices'])
        finally:
            mesh.close()
    assert counts[1] <= counts[0]


@pytest.mark.parametrize('name', sorted(SMALL))
def test_small_cases(name):
    v, f, K = SMALL[name]
    m = HM.fill(v, f, K)
    check_fill(m, raw_fill(v, f, K))
    check_independent(v, f, m)
    again = raw_fill(v, m['faces'], K)                                  # idempotent: nothing filled, the same face bytes
    assert again[0] == 0 and again[5][3] == 0 and np.array_equal(again[1][:3 * len(m['faces'])].reshape(-1, 3), m['faces'])


@pytest.mark.parametrize('name', sorted(LONG))
def test_long_loops(name):
    v, f, K = LONG[name]
    m = HM.fill(v, f, K)
    got = raw_fill(v, f, K)
    print('%s: report %s area %r' % (name, got[5][:12].tolist(), got[4][:1].tolist()))
    check_fill(m, got)
    check_independent(v, f, m)
    assert m['report'][3] == (0 if 'left' in name else 1) and m['report'][5] == (1 if 'left' in name else 0)


def test_optional_outputs_may_be_null():
    v, f, K = SMALL['permuted']
    check_fill(HM.fill(v, f, K), raw_fill(v, f, K, optional=False), optional=False)


def test_many_holes_and_determinism():
    v, f, K, m = many()
    assert m['report'][2] == 300 and m['report'][3] > 150 and m['report'][5] > 50
    a = raw_fill(v, f, K)
    check_fill(m, a)
    b = raw_fill(v, f, K)
    for x, y in zip(a[1:5], b[1:5]):
        assert x.tobytes() == y.tobytes()
    assert a[5].tolist() == b[5].tolist()
    check_independent(v, f, m)
    m40 = HM.fill(v, f, 40)                                             # both kernels in one call: loops up to 32 and beyond
    assert m40['report'][3] == 300 and m40['report'][10] > 32
    check_fill(m40, raw_fill(v, f, 40))
    again = raw_fill(v, m40['faces'], 40)
    assert again[0] == 0 and again[5][1:5].tolist() == [len(m40['faces']), 0, 0, 0]
    assert np.array_equal(again[1][:3 * len(m40['faces'])].reshape(-1, 3), m40['faces'])


def test_capacity_refusal_fills_the_report_and_writes_nothing():
    from points2surf_amd import holes
    v, f, K, m = many()
    nf, nh = len(m['faces']), len(m['holes'])
    for cf, ch in ((nf - 1, nh), (nf, nh - 1)):
        rc, fo, fs, ho, ha, rep = raw_fill(v, f, K, cap_faces=cf, cap_holes=ch)
        assert rc == P2S_EINVAL and rep[:12].tolist() == m['report'][:12].tolist()
        assert np.all(fo == -77) and np.all(fs == -77) and np.all(ho == -77) and np.all(ha == 77.0)
    check_fill(m, raw_fill(v, f, K, cap_faces=nf, cap_holes=nh))
    check_fill(m, raw_fill(v, f, K, cap_faces=nf, cap_holes=0, optional=False), optional=False)      # cap_holes counts only with its outputs
    # the Python call starts below what this mesh needs (more than 256 loops; many faces added) and repeats with the exact counts
    vo, fo, rep = holes.fill(v, f, max_hole_edges=40, want_map=True, want_holes=True)
    m40 = HM.fill(v, f, 40)
    assert rep['loops_found'] == 300 > 256 and rep['faces_added'] > len(f) // 16 + 1024
    assert vo.cpu().numpy().tobytes() == v.tobytes() and np.array_equal(fo.cpu().numpy(), m40['faces'])
    assert np.array_equal(rep['face_src'].cpu().numpy(), m40['face_src']) and np.array_equal(rep['holes'].cpu().numpy(), m40['holes'])
    assert rep['hole_area'].cpu().numpy().tobytes() == m40['hole_area'].tobytes()
    assert holes.report_dict(m40['report']) == {k: rep[k] for k in holes.REPORT_KEYS}


def test_invalid_meshes_are_refused():
    from points2surf_amd import _lib
    v, f, K = SMALL['loop5']
    for bad, word in (([0, 1, 500], b'out of range'), ([0, -1, 2], b'out of range'), ([0, 1, 1], b'repeated'), ([2, 1, 2], b'repeated')):
        g = f.copy()
        g[1] = bad
        got = raw_fill(v, g, K)
        assert got[0] == P2S_EINVAL and word in _lib.load().p2s_last_error() and np.all(got[1] == -77) and np.all(got[3] == -77)
    nan = v.copy()
    nan[2, 1] = np.nan
    assert raw_fill(nan, f, K)[0] == P2S_EINVAL and b'non-finite' in _lib.load().p2s_last_error()


def _voxel_bound(v, closed, g, m, res):
    """how many voxel centres the filled sphere and the uncut one may disagree on, from the model alone.  The two solids differ
    by the regions between the removed faces of a hole and its patch.  Such a region lies in the convex hull of their vertices,
    so in their bounding box and in the unit ball; it does not hold the origin, so the segment from the origin to one of its
    points crosses one of those faces first, and the point is no nearer to the origin than the nearest of their planes."""
    P = v.astype(np.float64)
    loops = HM.loops(g, len(v))
    kept = {tuple(t) for t in g.tolist()}
    removed = [t for t in closed.tolist() if tuple(t) not in kept]
    owner = {x: h for h, loop in enumerate(loops) for x in loop}
    pending = removed
    while pending:                                                      # a removed face belongs to the hole that it touches
        rest = []
        for t in pending:
            hs = {owner[x] for x in t if x in owner}
            assert len(hs) <= 1
            if hs:
                owner.update({x: next(iter(hs)) for x in t})
            else:
                rest.append(t)
        assert len(rest) < len(pending)
        pending = rest
    c = ((np.arange(res, dtype=np.float64) + 0.5) / res) * 2 - 1
    X, Y, Z = np.meshgrid(c, c, c, indexing='ij')
    R = np.sqrt(X * X + Y * Y + Z * Z)
    differ = np.zeros(R.shape, bool)
    for h, (v0, n, first, why) in enumerate(m['holes'].tolist()):
        assert why == HM.FILLED and loops[h][0] == v0
        tris = [t for t in removed if owner[t[0]] == h] + m['faces'][first:first + n - 2].tolist()
        pts = P[sorted({x for t in tris for x in t})]
        rho = 1.0
        for a, b, cc in tris:
            nrm = np.cross(P[b] - P[a], P[cc] - P[a])
            assert np.linalg.norm(nrm) > 0
            rho = min(rho, abs(nrm @ P[a]) / np.linalg.norm(nrm))
        lo, hi = pts.min(axis=0) - 1e-9, pts.max(axis=0) + 1e-9
        differ |= (X >= lo[0]) & (X <= hi[0]) & (Y >= lo[1]) & (Y <= hi[1]) & (Z >= lo[2]) & (Z <= hi[2]) & (R >= rho - 1e-9) & (R <= 1 + 1e-9)
    return int(differ.sum())


def test_a_sphere_with_six_holes_becomes_a_volume():
    from points2surf_amd import _lib, gt_sdf, holes
    v, closed, g = HM.sphere_with_holes()
    m = HM.fill(v, g, 60)
    bound = _voxel_bound(v, closed, g, m, 32)
    counts = {}
    for name, faces in (('closed', closed), ('cut', g), ('filled', holes.fill(v, g, max_hole_edges=60)[1].cpu().numpy())):
        mesh = gt_sdf.TriMesh(v, faces)
        try:
            if name == 'cut':
                with pytest.raises(_lib.P2SError):
                    mesh.voxelize(32)
            else:
                counts[name] = int(mesh.voxelize(32).sum())
        finally:
            mesh.close()
    print('voxels: closed %d, filled %d, bound on the difference %d' % (counts['closed'], counts['filled'], bound))
    assert 0 < bound and abs(counts['closed'] - counts['filled']) <= bound


def test_manifold_remove_with_area_fill():
    """two tetrahedra that share an edge (of four faces): mode 1 takes two of the four away, and --edges remove --fill area
    closes what that leaves: no edge of more than two faces, no non-manifold vertex, no boundary"""
    import manifold_model as MM
    from points2surf_amd import gt_sdf, manifold
    v, f = MM.small_cases()['tetras_sharing_an_edge']
    assert MM.defects(f)[0] == 1
    vo, fo, rep = manifold.remove_fill_split(v, f, max_hole_edges=100, fill='area')
    vo, fo = vo.cpu().numpy(), fo.cpu().numpy()
    assert MM.defects(fo) == (0, 0) and rep['boundary_edges_out'] == 0 == len(HM.boundary(fo)) and rep['faces_out'] == len(fo)
    assert rep['fill']['holes_filled'] >= 1 and rep['fill']['faces_added'] >= 1 and rep['repair']['holes_filled'] == 0
    mesh = gt_sdf.TriMesh(vo, fo)
    try:
        assert mesh.check()['nonmanifold_vertices'] == 0
    finally:
        mesh.close()
    row = manifold._row('x', 'remove+area', rep)
    assert (row['holes_filled'], row['faces_added'], row['verdict']) == (rep['fill']['holes_filled'], rep['fill']['faces_added'], 'closed')


def test_holes_command_line(tmp_path, capsys):
    from points2surf_amd import holes, ply
    indir, out = tmp_path / 'in', tmp_path / 'out'
    indir.mkdir()
    ply.write_ply(str(indir / 'whole.ply'), *HM.octahedron())
    v, f, _ = SMALL['limit_7']
    ply.write_ply(str(indir / 'cups.ply'), v, f)
    (indir / 'broken.ply').write_text('ply\nnot a mesh\n')
    assert holes.main(['--indir', str(indir), '--outdir', str(out), '--max_hole_edges', '7']) == 0
    with open(out / 'holes_report.csv', newline='') as fh:
        rows = {r['mesh']: r for r in csv.DictReader(fh)}
    assert list(rows['whole.ply']) == list(holes.REPORT_COLUMNS) and sorted(rows) == ['broken.ply', 'cups.ply', 'whole.ply']
    assert rows['broken.ply']['verdict'].startswith('failed: ') and not os.path.exists(out / 'broken.ply')
    m = HM.fill(v, f, 7)
    c, w = rows['cups.ply'], rows['whole.ply']
    assert (c['max_hole_edges'], c['loops_found'], c['holes_filled'], c['faces_added'], c['loops_too_long'], c['boundary_edges_out'],
            c['verdict']) == ('7', '3', '2', '6', '1', '12', 'open')
    assert (w['faces_in'], w['faces_out'], w['loops_found'], w['verdict']) == ('8', '8', '0', 'closed')
    gv, gf = ply.read_ply(str(out / 'cups.ply'))
    assert np.asarray(gv, np.float32).tobytes() == v.tobytes() and np.array_equal(np.asarray(gf).reshape(-1, 3), m['faces'])
    # a second run: both up to date, the rows kept; the broken one is tried again
    stamp = os.path.getmtime(out / 'cups.ply')
    os.utime(indir / 'cups.ply', (1, 1))
    os.utime(indir / 'whole.ply', (1, 1))
    capsys.readouterr()
    assert holes.fill_dir(str(indir), str(out), max_hole_edges=7) == []
    assert capsys.readouterr().out.count('up to date') == 2 and os.path.getmtime(out / 'cups.ply') == stamp
    with open(out / 'holes_report.csv', newline='') as fh:
        assert {r['mesh']: r for r in csv.DictReader(fh)} == rows
    # another bound is not up to date; --dataset names the meshes
    (tmp_path / 'set.txt').write_text('cups\n')
    assert [os.path.basename(p) for p in holes.fill_dir(str(indir), str(out), max_hole_edges=30, dataset=str(tmp_path / 'set.txt'))] == ['cups.ply']
    with open(out / 'holes_report.csv', newline='') as fh:
        rows = list(csv.DictReader(fh))
    assert len(rows) == 1 and (rows[0]['holes_filled'], rows[0]['verdict']) == ('3', 'closed')
