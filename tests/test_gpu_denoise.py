"""p2s_mesh_denoise on the device (points2surf_amd/denoise.py) against the numpy model (tests/denoise_model.py) for EQUALITY
of bytes on every case: positions, target normals, classes, report [0..11]; nothing written beyond the outputs; the
simultaneous updates on meshes larger than a wave, a block and the grid stride of the class kernel; neighbours met in two and
in three rows of the merge; rows of thousands of faces; fixed vertices and the sign of their zeros; tiny coordinates; both ends
of the threshold; determinism; the refusals; the command line."""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest

import denoise_model as DM

pytestmark = pytest.mark.gpu

P2S_EINVAL = -1
PAD = 256
CASES = DM.class_cases()


def _dev():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def raw_denoise(v, f, T, nit, vit, mode, fixed=None, want_class=True, want_normals=True, out='own'):
    """the raw call with the three outputs filled with a pattern first and PAD entries of it behind
    -> rc, positions, normals, classes, report"""
    import torch
    from points2surf_amd import _lib, engine
    lib, dev = _lib.load(), _dev()
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    V, F = len(v), len(f)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    tx = torch.from_numpy(np.ascontiguousarray(fixed, np.uint8)).to(dev) if fixed is not None else None
    vo = torch.full((3 * V + PAD,), -77.0, dtype=torch.float32, device=dev)
    no = torch.full((3 * F + PAD,), -55.0, dtype=torch.float32, device=dev)
    co = torch.full((V + PAD,), 77, dtype=torch.uint8, device=dev)
    rep = (ctypes.c_int64 * 16)(*([-1] * 16))
    ptr = lambda t, n: engine._ptr(t) if t is not None and n else None
    rc = lib.p2s_mesh_denoise(ptr(tv, V), V, ptr(tf, F), F, T, nit, vit, mode, ptr(tx, V), engine._ptr(tv if out == 'alias' else vo),
                              engine._ptr(no) if want_normals else None, engine._ptr(co) if want_class else None, rep, dev.index,
                              engine._stream_ptr(dev))
    torch.cuda.synchronize()
    assert tv.cpu().numpy().tobytes() == v.tobytes() and tf.cpu().numpy().tobytes() == f.tobytes()      # the input is read only
    return rc, vo.cpu().numpy(), no.cpu().numpy(), co.cpu().numpy(), np.array(rep[:], np.int64)


def untouched(got):
    return np.all(got[1] == -77.0) and np.all(got[2] == -55.0) and np.all(got[3] == 77)


def check(m, got, want_class=True, want_normals=True):
    rc, vo, no, co, rep = got
    V, F = len(m['verts']), len(m['normals'])
    assert rc == 0 == m['rc']
    assert rep[:12].tolist() == m['report'][:12].tolist() and rep[12:].tolist() == [0, 0, 0, 0]
    assert no[:3 * F].tobytes() == m['normals'].tobytes() if want_normals else np.all(no == -55.0)
    assert np.all(no[3 * F:] == -55.0)
    assert vo[:3 * V].tobytes() == m['verts'].tobytes() and np.all(vo[3 * V:] == -77.0)
    assert co[:V].tobytes() == m['cls'].tobytes() if want_class else np.all(co == 77)
    assert np.all(co[V:] == 77)


def both(v, f, T=0.5, nit=10, vit=10, mode=0, fixed=None, want_class=True, want_normals=True):
    m = DM.denoise(v, f, T, nit, vit, mode, fixed)
    check(m, raw_denoise(v, f, T, nit, vit, mode, fixed, want_class, want_normals), want_class, want_normals)
    return m


@pytest.mark.parametrize('name', sorted(CASES))
def test_class_cases(name):
    v, f, fixed, want = CASES[name]
    for mode in (0, 1):
        for want_class, want_normals in ((True, True), (False, True), (True, False), (False, False)):
            m = both(v, f, 0.5, 2, 2, mode, fixed, want_class, want_normals)
            assert m['cls'].tolist() == want[mode]
    m = both(v, f, 0.0, 3, 3, 1, fixed)                                 # T = 0: the faces of the tetrahedron still do not mix, the sheet's do
    assert m['cls'].tolist() == want[1]


@functools.lru_cache(maxsize=None)
def solid(name):
    return dict(tetrahedron=DM.tetrahedron, octahedron=DM.octahedron, icosphere=lambda: DM.icosphere(3, noise=0.02, seed=7))[name]()


@pytest.mark.parametrize('name', ['tetrahedron', 'octahedron', 'icosphere'])
def test_closed_meshes(name):
    """every face of a tetrahedron neighbours every face; on the octahedron all but the opposite one"""
    v, f = solid(name)
    if name != 'icosphere':
        v = v + np.random.default_rng(8).normal(0.0, 0.05, v.shape).astype(np.float32)
    for T in (0.0, 0.5):
        for nit, vit in ((1, 1), (3, 2), (10, 10)):
            m = both(v, f, T, nit, vit, 0)
            assert m['report'][1] == len(v) and m['report'][8:10].tolist() == [nit, vit]
    assert m['report'][7] == dict(tetrahedron=4, octahedron=7, icosphere=13)[name]
    assert name != 'icosphere' or m['verts'].tobytes() != v.tobytes()


def test_a_neighbour_met_in_two_and_in_three_rows_counts_once():
    v = np.array([[0, 0, 0], [1, 0, 0.1], [0, 1, -0.1], [1, 1, 0.3]], np.float32)
    pair = both(v, [[0, 1, 2], [2, 1, 3]], 0.0, 3, 3, 1)                # two triangles on an edge: the other one heads two rows
    assert pair['report'][7] == 2 and pair['normals'][0].tobytes() != DM.face_normals(v, np.array([[0, 1, 2]]))[0].tobytes()
    twin = both(v[:3], [[0, 1, 2], [0, 2, 1]], 0.0, 3, 3, 1)            # a face and its flipped twin: each heads all three rows
    assert twin['report'][7] == 2 and twin['normals'][0].tobytes() == (-twin['normals'][1]).tobytes()
    both(v[:3], [[0, 1, 2], [0, 1, 2], [1, 2, 0]], 0.0, 2, 2, 1)        # the same face three times, one with its corners rotated


@pytest.mark.parametrize('n', [17, 65])
@pytest.mark.parametrize('iterations', [(1, 1), (2, 3), (10, 10), (0, 5), (5, 0)])
def test_open_grids_pin_the_simultaneous_updates(n, iterations):
    """an update in place, or one that reads a half-written buffer, shows on any mesh larger than a wave: 8,192 faces and 4,225
    vertices are more than one block and no multiple of 256; an even and an odd count end in either ping-pong buffer"""
    v, f = DM.grid(n, n, noise=0.2, seed=n)
    for mode in (0, 1):
        m = both(v, f, 0.5, *iterations, mode)
        assert m['report'][1] == ((n - 2) ** 2 if mode == 0 else n * n) and m['report'][8:10].tolist() == list(iterations)
        assert (m['verts'].tobytes() == v.tobytes()) == (iterations[1] == 0)


def test_more_vertices_than_the_class_kernels_grid_covers_in_one_stride():
    v, f = DM.grid(259, 259, noise=0.2, seed=5)                         # 67,081 vertices > 256 workgroups of 256
    assert both(v, f, 0.4, 2, 2, 0)['report'][1] == 257 * 257


def test_an_apex_fan_with_long_rows():
    v, f = DM.fan(3000)
    m = both(v, f, 0.5, 2, 2, 1)
    assert m['report'][7] == 3000 and m['report'][1] == 3001


def test_a_mask_keeps_bytes_and_the_sign_of_zero():
    v, f = DM.icosphere(2, noise=0.05, seed=11)
    fixed = (np.arange(len(v)) % 3 == 0).astype(np.uint8)
    v[0] = [-0.0, 0.0, -0.0]
    v[4, 1] = -0.0                                                      # and one that moves
    m = both(v, f, 0.3, 4, 4, 0, fixed)
    assert m['verts'][fixed != 0].tobytes() == v[fixed != 0].tobytes() and m['report'][3] == int(fixed.sum())
    assert np.signbit(m['verts'][0]).tolist() == [True, False, True]
    both(v, f, 0.3, 4, 4, 1, fixed * 5)                                 # any nonzero byte masks
    g, gf = DM.grid(9, 9, noise=0.2, seed=3)                            # boundary vertices of mode 0 keep a -0.0 too
    g[0] = [-0.0, -0.0, 0.0]
    assert np.signbit(both(g, gf, 0.3, 3, 3, 0)['verts'][0]).tolist() == [True, True, False]


def test_tiny_coordinates_still_give_unit_normals():
    v, f = DM.icosphere(2, noise=0.05, seed=12)
    tiny = v * np.float32(1e-30)
    m = both(tiny, f, 0.5, 3, 3, 0)
    assert m['report'][6] == 0 and np.allclose(np.linalg.norm(m['normals'].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.any(m['verts'] != tiny)
    far = both(v + np.float32(1e3), f, 0.5, 3, 3, 0)                    # float64 sums: positions near 1,000 still move
    assert np.any(far['verts'] != v + np.float32(1e3))
    g = DM.grid(9, 9, noise=0.2, seed=13)
    both(g[0] * np.float32(1e-39), g[1], 0.5, 3, 3, 1)                  # subnormal input: nothing is flushed on the way


@pytest.mark.parametrize('T', [0.0, 0.999])
def test_both_ends_of_the_threshold(T):
    v, f = DM.icosphere(3, noise=0.02, seed=15)
    m = both(v, f, T, 5, 5, 0)
    geometric = DM.face_normals(v, f)
    assert m['normals'].tobytes() != geometric.tobytes()                # at 0.999 a face still sees itself: renormalised at least
    c, cf, _ = DM.noisy_cube(4)
    both(c, cf, T, 5, 5, 0)


def test_two_runs_give_equal_bytes():
    v, f = DM.grid(120, 120, noise=0.2, seed=9)
    a = raw_denoise(v, f, 0.5, 10, 10, 0)
    b = raw_denoise(v, f, 0.5, 10, 10, 0)
    assert a[0] == 0 == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    check(DM.denoise(v, f, 0.5, 10, 10, 0), a)


def test_nothing_to_do_copies_the_input():
    v, f = DM.icosphere(1, noise=0.05, seed=14)
    v[2, 0] = -0.0
    for nit, vit, faces in ((0, 0, f), (5, 5, f[:0]), (0, 0, f[:0]), (4, 0, f)):
        for mode in (0, 1):
            m = both(v, faces, 0.5, nit, vit, mode)
            assert m['verts'].tobytes() == v.tobytes() and m['report'][9] == 0 and m['report'][10] == 0
    both(v[:0], f[:0], 0.5, 3, 3, 0)                                    # no vertex at all
    fixed = np.ones(len(v), np.uint8)                                   # every vertex masked: normals filtered, no vertex iteration
    assert both(v, f, 0.5, 5, 5, 0, fixed)['report'][8:10].tolist() == [5, 0]


def test_invalid_input_is_refused_and_nothing_is_written():
    from points2surf_amd import _lib
    v, f = DM.icosphere(1)
    for bad, word in (([0, 1, 500], b'out of range'), ([0, -1, 2], b'out of range'), ([0, 1, 1], b'repeated'), ([2, 1, 2], b'repeated')):
        g = f.copy()
        g[1] = bad
        got = raw_denoise(v, g, 0.5, 2, 2, 0)
        assert got[0] == P2S_EINVAL and word in _lib.load().p2s_last_error() and untouched(got)
    nan = v.copy()
    nan[2, 1] = np.nan
    got = raw_denoise(nan, f, 0.5, 2, 2, 0)
    assert got[0] == P2S_EINVAL and b'non-finite' in _lib.load().p2s_last_error() and untouched(got)
    got = raw_denoise(v, f, 0.5, 2, 2, 0, out='alias')                  # raw_denoise itself asserts that the input kept its bytes
    assert got[0] == P2S_EINVAL and b'verts_out_dev' in _lib.load().p2s_last_error() and untouched(got)
    for kw, word in ((dict(T=1.0), b'threshold'), (dict(nit=-1), b'normal_iterations'), (dict(vit=-1), b'vertex_iterations'),
                     (dict(mode=2), b'boundary_mode')):
        a = dict(T=0.5, nit=2, vit=2, mode=0)
        a.update(kw)
        got = raw_denoise(v, f, a['T'], a['nit'], a['vit'], a['mode'])
        assert got[0] == P2S_EINVAL and word in _lib.load().p2s_last_error() and untouched(got)
        assert got[4].tolist() == [-1] * 16


def test_overflow_of_a_vertex_step_fails_with_the_report_filled():
    from points2surf_amd import _lib
    # a flat face at the top of the float32 range beside a steep one: the filter tilts its normal by 0.002, and vertex 0,
    # 4e38 away from the face's centroid, rises by 4e38 * 0.002 above the largest float
    big = np.array([[-3e38, 0, 3.4e38], [3e38, -1e38, 3.4e38], [3e38, 1e38, 3.4e38], [3.3e38, 0, -3e38]], np.float32)
    f = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    m = DM.denoise(big, f, 0.0, 1, 1, 1)
    got = raw_denoise(big, f, 0.0, 1, 1, 1)
    assert m['rc'] == P2S_EINVAL and m['report'][11] == 1 and np.isinf(m['verts'][0, 2])
    assert got[0] == P2S_EINVAL and b'not finite' in _lib.load().p2s_last_error()
    assert got[4][:12].tolist() == m['report'][:12].tolist() and got[4][12:].tolist() == [0, 0, 0, 0] and untouched(got)
    both(big, f, 0.0, 1, 0, 1)                                          # the normal iteration alone stays finite


def test_python_call():
    from points2surf_amd import denoise
    v, f = DM.grid(17, 17, noise=0.2, seed=17)
    fixed = np.arange(len(v)) % 7 == 0
    for boundary in denoise.BOUNDARY_MODES:
        m = DM.denoise(v, f, mode=DM.MODES[boundary], fixed=fixed)
        vo, fo, rep = denoise.denoise(v, f, boundary=boundary, fixed=fixed, want_class=True, want_normals=True)
        assert vo.cpu().numpy().tobytes() == m['verts'].tobytes() and np.array_equal(fo.cpu().numpy(), f)
        assert rep['class'].cpu().numpy().tobytes() == m['cls'].tobytes()
        assert rep['normals'].cpu().numpy().tobytes() == m['normals'].tobytes()
        assert denoise.report_dict(m['report']) == {k: rep[k] for k in denoise.REPORT_KEYS}
    rep = denoise.denoise(v, f)[2]
    assert 'class' not in rep and 'normals' not in rep


def test_denoise_command_line(tmp_path, capsys):
    from points2surf_amd import denoise, ply
    indir, out = tmp_path / 'in', tmp_path / 'out'
    indir.mkdir()
    cv, cf, _ = DM.noisy_cube(6)
    gv, gf = DM.grid(9, 9, noise=0.2, seed=22)
    ply.write_ply(str(indir / 'cube.ply'), cv, cf)
    ply.write_ply(str(indir / 'sheet.ply'), gv, gf)
    (indir / 'broken.ply').write_text('ply\nnot a mesh\n')
    assert denoise.main(['--indir', str(indir), '--outdir', str(out), '--threshold', '0.4', '--normal_iterations', '4',
                         '--vertex_iterations', '5', '--boundary', 'free']) == 0
    with open(out / 'denoise_report.csv', newline='') as fh:
        rows = {r['mesh']: r for r in csv.DictReader(fh)}
    assert list(rows['cube.ply']) == list(denoise.REPORT_COLUMNS) and sorted(rows) == ['broken.ply', 'cube.ply', 'sheet.ply']
    assert rows['broken.ply']['verdict'].startswith('failed: ') and not os.path.exists(out / 'broken.ply')
    for name, v, f in (('cube', cv, cf), ('sheet', gv, gf)):
        m = DM.denoise(v, f, 0.4, 4, 5, 1)
        r = rows[name + '.ply']
        assert (r['threshold'], r['normal_iterations'], r['vertex_iterations'], r['boundary'], r['verdict']) == ('0.4', '4', '5', 'free',
                                                                                                                'denoised')
        assert [int(r[k]) for k in denoise.REPORT_KEYS[2:11]] == m['report'][1:10].tolist()
        pv, pf = ply.read_ply(str(out / (name + '.ply')))
        assert np.asarray(pv, np.float32).tobytes() == m['verts'].tobytes() and np.array_equal(np.asarray(pf).reshape(-1, 3), f)
    c = rows['cube.ply']
    import smooth_model as SM
    vol_in, vol_out = SM.signed_volume(cv, cf), SM.signed_volume(DM.denoise(cv, cf, 0.4, 4, 5, 1)['verts'], cf)
    assert float(c['volume_in']) == pytest.approx(vol_in, rel=1e-5) and float(c['volume_out']) == pytest.approx(vol_out, rel=1e-5)
    assert float(c['area_in']) > float(c['area_out']) > 0 and float(rows['sheet.ply']['area_in']) > 0
    # a second run: both up to date, the rows kept; the broken one is tried again
    stamp = os.path.getmtime(out / 'cube.ply')
    os.utime(indir / 'cube.ply', (1, 1))
    os.utime(indir / 'sheet.ply', (1, 1))
    capsys.readouterr()
    kw = dict(threshold=0.4, normal_iterations=4, vertex_iterations=5, boundary='free')
    assert denoise.denoise_dir(str(indir), str(out), **kw) == []
    assert capsys.readouterr().out.count('up to date') == 2 and os.path.getmtime(out / 'cube.ply') == stamp
    with open(out / 'denoise_report.csv', newline='') as fh:
        assert {r['mesh']: r for r in csv.DictReader(fh)} == rows
    # other settings are not up to date; --dataset names the meshes
    (tmp_path / 'set.txt').write_text('sheet\n')
    kw['threshold'] = 0.5
    assert [os.path.basename(p) for p in denoise.denoise_dir(str(indir), str(out), dataset=str(tmp_path / 'set.txt'), **kw)] == ['sheet.ply']
    with open(out / 'denoise_report.csv', newline='') as fh:
        rows = list(csv.DictReader(fh))
    assert len(rows) == 1 and (rows[0]['threshold'], rows[0]['normal_iterations_run'], rows[0]['verdict']) == ('0.5', '4', 'denoised')
