"""p2s_mesh_smooth on the device (points2surf_amd/smooth.py) against the numpy model (tests/smooth_model.py) for EQUALITY of
bytes on every case: positions, classes, report [0..11]; nothing written beyond the vertices; the simultaneous update on meshes
larger than a wave and than a block; rows of thousands of neighbours; fixed vertices and the sign of their zeros; float64 sums
and subnormal results; determinism; face order; the refusals; the command line."""
import csv
import ctypes
import functools
import os

import numpy as np
import pytest

import smooth_model as SM

pytestmark = pytest.mark.gpu

P2S_EINVAL = -1
PAD = 256
CASES = SM.class_cases()
TAUBIN = (0.5, -0.53)


def _dev():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def raw_smooth(v, f, it, lam, mu, mode, fixed=None, want_class=True, out='own'):
    """the raw call with both outputs filled with a pattern first and PAD entries of it behind -> rc, positions, classes, report"""
    import torch
    from points2surf_amd import _lib, engine
    lib, dev = _lib.load(), _dev()
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    V, F = len(v), len(f)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    tx = torch.from_numpy(np.ascontiguousarray(fixed, np.uint8)).to(dev) if fixed is not None else None
    vo = torch.full((3 * V + PAD,), -77.0, dtype=torch.float32, device=dev)
    co = torch.full((V + PAD,), 77, dtype=torch.uint8, device=dev)
    rep = (ctypes.c_int64 * 16)(*([-1] * 16))
    ptr = lambda t, n: engine._ptr(t) if t is not None and n else None
    rc = lib.p2s_mesh_smooth(ptr(tv, V), V, ptr(tf, F), F, it, lam, mu, mode, ptr(tx, V), engine._ptr(tv if out == 'alias' else vo),
                             engine._ptr(co) if want_class else None, rep, dev.index, engine._stream_ptr(dev))
    torch.cuda.synchronize()
    assert tv.cpu().numpy().tobytes() == v.tobytes()                    # the input is read only
    return rc, vo.cpu().numpy(), co.cpu().numpy(), np.array(rep[:], np.int64)


def check(m, got, want_class=True):
    rc, vo, co, rep = got
    V = len(m['verts'])
    assert rc == 0 == m['rc']
    assert rep[:12].tolist() == m['report'][:12].tolist() and rep[12:].tolist() == [0, 0, 0, 0]
    assert vo[:3 * V].tobytes() == m['verts'].tobytes() and np.all(vo[3 * V:] == -77.0)
    if want_class:
        assert co[:V].tobytes() == m['cls'].tobytes() and np.all(co[V:] == 77)
    else:
        assert np.all(co == 77)


def both(v, f, it, lam, mu, mode, fixed=None, want_class=True):
    m = SM.smooth(v, f, it, lam, mu, mode, fixed)
    check(m, raw_smooth(v, f, it, lam, mu, mode, fixed, want_class), want_class)
    return m


@pytest.mark.parametrize('name', sorted(CASES))
def test_class_cases(name):
    v, f, fixed, want = CASES[name]
    for mode in (0, 1, 2):
        for want_class in (True, False):
            m = both(v, f, 2, *TAUBIN, mode, fixed, want_class)
            assert m['cls'].tolist() == want[mode]


@functools.lru_cache(maxsize=None)
def solid(name):
    return dict(tetrahedron=SM.tetrahedron, octahedron=SM.octahedron, icosphere=lambda: SM.icosphere(3, noise=0.02, seed=7))[name]()


@pytest.mark.parametrize('name', ['tetrahedron', 'octahedron', 'icosphere'])
@pytest.mark.parametrize('iterations', [1, 2, 10])
def test_closed_meshes(name, iterations):
    v, f = solid(name)
    for lam, mu in (TAUBIN, (0.5, 0.0), (1.0, -2.0)):
        m = both(v, f, iterations, lam, mu, 0)
        assert m['report'][1] == len(v) and m['report'][9] == iterations * (2 if mu else 1)


@pytest.mark.parametrize('n', [17, 65])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_open_grids_pin_the_simultaneous_update(n, mode):
    """an update in place, or one that reads a half-written buffer, shows on any mesh larger than a wave: 4,225 vertices are
    more than one block and no multiple of 256"""
    v, f = SM.grid(n, n, noise=0.2, seed=n)
    m = both(v, f, 3, *TAUBIN, mode)
    assert m['report'][1 + (1 if mode == 1 else 0)] > 0 and (mode == 2 or m['report'][1] == (n - 2) ** 2)


def test_cone_with_a_long_row():
    v, f = SM.cone(3000)
    m = both(v, f, 2, *TAUBIN, 0)
    assert m['report'][8] == 3000 and m['report'][1] == 3002
    both(v, f, 1, 0.5, 0.0, 0, fixed=(np.arange(3002) == 3000).astype(np.uint8))      # one apex masked: one long row left
    v65, f65 = SM.cone(65)                                              # rows of a wave's width, and one more
    v64, f64 = SM.cone(64)
    assert both(v64, f64, 2, *TAUBIN, 0)['report'][8] == 64 and both(v65, f65, 2, *TAUBIN, 0)['report'][8] == 65
    for n in (129, 256, 257, 513):
        assert both(*SM.cone(n), 1, *TAUBIN, 0)['report'][8] == n


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257])
def test_vertex_counts_at_the_wave_and_block_edges(n):
    v, f = SM.strip(n, seed=n)
    both(v, f, 2, *TAUBIN, 2)
    both(v, f, 2, *TAUBIN, 1)


def test_a_mask_keeps_bytes_and_the_sign_of_zero():
    v, f = SM.icosphere(2, noise=0.05, seed=11)
    fixed = (np.arange(len(v)) % 3 == 0).astype(np.uint8)
    v[0] = [-0.0, 0.0, -0.0]
    v[4, 1] = -0.0                                                      # and one that moves
    m = both(v, f, 4, *TAUBIN, 0, fixed)
    assert m['verts'][fixed != 0].tobytes() == v[fixed != 0].tobytes() and m['report'][5] == int(fixed.sum())
    assert np.signbit(m['verts'][0]).tolist() == [True, False, True]
    both(v, f, 4, *TAUBIN, 1, fixed * 5)                                # any nonzero byte masks


def test_float64_sums_and_subnormal_results():
    v, f = SM.icosphere(2, noise=0.05, seed=12)
    far = both(v + np.float32(1e6), f, 3, *TAUBIN, 0)
    assert not np.array_equal(far['verts'], v + np.float32(1e6))
    tiny = v * np.float32(1e-30)
    m = both(tiny, f, 3, *TAUBIN, 0)
    g = SM.grid(9, 9, noise=0.2, seed=13)
    sub = both(g[0] * np.float32(1e-39), g[1], 3, *TAUBIN, 2)            # subnormal input and output: nothing is flushed
    assert np.any(m['verts'] != 0) and np.any((sub['verts'] != 0) & (np.abs(sub['verts']) < np.float32(1.1754944e-38)))


def test_a_large_grid_two_calls_and_shuffled_faces():
    v, f = SM.grid(200, 200, noise=0.2, seed=9)
    m = SM.smooth(v, f, 10, *TAUBIN, 0)
    a = raw_smooth(v, f, 10, *TAUBIN, 0)
    check(m, a)
    b = raw_smooth(v, f, 10, *TAUBIN, 0)
    c = raw_smooth(v, SM.shuffled(f, 4), 10, *TAUBIN, 0)
    for other in (b, c):
        assert other[0] == 0 and other[1].tobytes() == a[1].tobytes() and other[2].tobytes() == a[2].tobytes()
        assert other[3].tolist() == a[3].tolist()


def test_nothing_to_do_copies_the_input():
    v, f = SM.icosphere(1, noise=0.05, seed=14)
    v[2, 0] = -0.0
    for it, faces in ((0, f), (5, f[:0]), (0, f[:0])):
        for mode in (0, 1, 2):
            m = both(v, faces, it, *TAUBIN, mode)
            assert m['verts'].tobytes() == v.tobytes() and m['report'][9] == 0 and m['report'][10] == 0
    assert SM.smooth(v, f[:0], 5, *TAUBIN, 0)['cls'].tolist() == [5] * len(v)
    both(v[:0], f[:0], 3, *TAUBIN, 0)                                   # no vertex at all
    fixed = np.ones(len(v), np.uint8)                                   # every vertex masked: faces, iterations, and no half-step
    assert both(v, f, 5, *TAUBIN, 0, fixed)['report'][9] == 0


def test_invalid_input_is_refused_and_nothing_is_written():
    from points2surf_amd import _lib
    v, f = SM.icosphere(1)
    for bad, word in (([0, 1, 500], b'out of range'), ([0, -1, 2], b'out of range'), ([0, 1, 1], b'repeated'), ([2, 1, 2], b'repeated')):
        g = f.copy()
        g[1] = bad
        got = raw_smooth(v, g, 2, *TAUBIN, 0)
        assert got[0] == P2S_EINVAL and word in _lib.load().p2s_last_error() and np.all(got[1] == -77.0) and np.all(got[2] == 77)
    nan = v.copy()
    nan[2, 1] = np.nan
    got = raw_smooth(nan, f, 2, *TAUBIN, 0)
    assert got[0] == P2S_EINVAL and b'non-finite' in _lib.load().p2s_last_error() and np.all(got[1] == -77.0) and np.all(got[2] == 77)
    got = raw_smooth(v, f, 2, *TAUBIN, 0, out='alias')                  # raw_smooth itself asserts that the input kept its bytes
    assert got[0] == P2S_EINVAL and b'verts_out_dev' in _lib.load().p2s_last_error() and np.all(got[2] == 77)


def test_overflow_of_a_half_step_fails_with_the_report_filled():
    from points2surf_amd import _lib
    v, f = SM.tetrahedron()
    big = v * np.float32(3e38)
    m = SM.smooth(big, f, 1, 1.0, -2.0, 0)
    rc, vo, co, rep = raw_smooth(big, f, 1, 1.0, -2.0, 0)
    assert rc == P2S_EINVAL == m['rc'] and b'not finite' in _lib.load().p2s_last_error()
    assert rep[11] > 0 and rep[:12].tolist() == m['report'][:12].tolist() and np.all(vo == -77.0) and np.all(co == 77)
    both(big, f, 1, 1.0, 0.0, 0)                                        # the lambda half-step alone stays finite


def test_python_call():
    from points2surf_amd import smooth
    v, f = SM.grid(17, 17, noise=0.2, seed=17)
    fixed = np.arange(len(v)) % 7 == 0
    for boundary in smooth.BOUNDARY_MODES:
        m = SM.smooth(v, f, 10, *TAUBIN, SM.MODES[boundary], fixed)
        vo, fo, rep = smooth.smooth(v, f, boundary=boundary, fixed=fixed, want_class=True)
        assert vo.cpu().numpy().tobytes() == m['verts'].tobytes() and np.array_equal(fo.cpu().numpy(), f)
        assert rep['class'].cpu().numpy().tobytes() == m['cls'].tobytes()
        assert smooth.report_dict(m['report']) == {k: rep[k] for k in smooth.REPORT_KEYS}
    assert 'class' not in smooth.smooth(v, f)[2]


def test_smooth_command_line(tmp_path, capsys):
    from points2surf_amd import ply, smooth
    indir, out = tmp_path / 'in', tmp_path / 'out'
    indir.mkdir()
    sv, sf = SM.icosphere(2, noise=0.05, seed=21)
    gv, gf = SM.grid(9, 9, noise=0.2, seed=22)
    ply.write_ply(str(indir / 'ball.ply'), sv, sf)
    ply.write_ply(str(indir / 'sheet.ply'), gv, gf)
    (indir / 'broken.ply').write_text('ply\nnot a mesh\n')
    assert smooth.main(['--indir', str(indir), '--outdir', str(out), '--iterations', '4', '--boundary', 'curve']) == 0
    with open(out / 'smooth_report.csv', newline='') as fh:
        rows = {r['mesh']: r for r in csv.DictReader(fh)}
    assert list(rows['ball.ply']) == list(smooth.REPORT_COLUMNS) and sorted(rows) == ['ball.ply', 'broken.ply', 'sheet.ply']
    assert rows['broken.ply']['verdict'].startswith('failed: ') and not os.path.exists(out / 'broken.ply')
    for name, v, f in (('ball', sv, sf), ('sheet', gv, gf)):
        m = SM.smooth(v, f, 4, *TAUBIN, 1)
        r = rows[name + '.ply']
        assert (r['iterations'], r['lambda'], r['mu'], r['boundary'], r['verdict']) == ('4', '0.5', '-0.53', 'curve', 'smoothed')
        assert [int(r[k]) for k in smooth.REPORT_KEYS[2:11]] == m['report'][1:10].tolist()
        pv, pf = ply.read_ply(str(out / (name + '.ply')))
        assert np.asarray(pv, np.float32).tobytes() == m['verts'].tobytes() and np.array_equal(np.asarray(pf).reshape(-1, 3), f)
    b = rows['ball.ply']
    vol_in, vol_out = SM.signed_volume(sv, sf), SM.signed_volume(SM.smooth(sv, sf, 4, *TAUBIN, 1)['verts'], sf)
    assert float(b['volume_in']) == pytest.approx(vol_in, rel=1e-5) and float(b['volume_out']) == pytest.approx(vol_out, rel=1e-5)
    assert float(b['area_in']) > float(b['area_out']) > 0 and float(rows['sheet.ply']['area_in']) > 0
    # a second run: both up to date, the rows kept; the broken one is tried again
    stamp = os.path.getmtime(out / 'ball.ply')
    os.utime(indir / 'ball.ply', (1, 1))
    os.utime(indir / 'sheet.ply', (1, 1))
    capsys.readouterr()
    assert smooth.smooth_dir(str(indir), str(out), iterations=4, boundary='curve') == []
    assert capsys.readouterr().out.count('up to date') == 2 and os.path.getmtime(out / 'ball.ply') == stamp
    with open(out / 'smooth_report.csv', newline='') as fh:
        assert {r['mesh']: r for r in csv.DictReader(fh)} == rows
    # other settings are not up to date; --dataset names the meshes
    (tmp_path / 'set.txt').write_text('sheet\n')
    assert [os.path.basename(p) for p in smooth.smooth_dir(str(indir), str(out), iterations=4, mu=0.0, boundary='curve',
                                                           dataset=str(tmp_path / 'set.txt'))] == ['sheet.ply']
    with open(out / 'smooth_report.csv', newline='') as fh:
        rows = list(csv.DictReader(fh))
    assert len(rows) == 1 and (rows[0]['mu'], rows[0]['half_steps'], rows[0]['verdict']) == ('0.0', '4', 'smoothed')
