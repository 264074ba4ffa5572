"""Raw scans on the device (points2surf_amd.prepare: p2s_prepare_*) against the float64 model (tests/prepare_model.py).

Everything that selects is exact: bounds, ids, d_i, R, occupied cells and the normalised bytes equal the model's.  mean and std
come from a fixed tree of at most 4099 doubles (error below n 2^-53) against ``math.fsum``: 1e-12 and 1e-11 relative.  The keep
flags of the outlier stage are compared outside the band |d_i - threshold| <= 1e-9 threshold, which the seeds leave empty
(n = 2 is degenerate -- both d_i equal the threshold -- and is compared through the exact mean instead)."""
import csv
import functools
import os

import numpy as np
import pytest
import torch

import prepare_model as M

pytestmark = pytest.mark.gpu

SIZES = M.SIZES                                      # 257: one past a block; 4099: several blocks, no power of two
BAND = 1e-9


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- the compaction behind every selecting stage ------------------------------------------------------------------------

# pp_compact scans its per-block counts IN PLACE with the shared one-workgroup scan (p2s_scan_kernel), which walks them in chunks
# of 1024 with a carry.  A block is 256 points: 1 / 255 / 256 / 257 are one block, its last point, and the second block;
# 262143 / 262144 / 262145 are 1024 blocks (one chunk, exactly) and 1025 (the second chunk and its carry).
@pytest.mark.parametrize('n', (1, 255, 256, 257, 262143, 262144, 262145))
def test_compaction_scans_in_place_across_its_chunks(n):
    from points2surf_amd import prepare
    i = np.arange(n)
    rows = np.stack([i, -i, 0.5 * i], axis=1).astype(np.float32)           # exact below 2^24: every row names its index
    patterns = {'all': np.ones(n, bool), 'none': np.zeros(n, bool), 'every third': i % 3 == 0, 'all but every third': i % 3 != 0}
    for name, keep in patterns.items():
        p = rows.copy()
        p[~keep, (i % 3)[~keep]] = np.where(i[~keep] % 2 == 0, np.nan, np.inf)       # one non-finite coordinate drops the row
        out, ids = prepare.drop_nonfinite(p)
        assert out.shape == (int(keep.sum()), 3) and ids.shape == (int(keep.sum()),), name       # the count that was returned
        assert ids.dtype == torch.int32 and np.array_equal(_np(ids), np.flatnonzero(keep)), name
        assert _same_bytes(_np(out), rows[keep]), name


# ---- crop ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('q', (0.01, 0.1, 0.49))
@pytest.mark.parametrize('n', SIZES)
def test_crop_bounds_and_ids(n, q):
    from points2surf_amd import prepare
    p = M.seeded_cloud(n, seed=1)
    want_ids, want_b = M.crop(p, q, 0.25)
    out, ids, rep = prepare.crop(p, q, 0.25, want_report=True)
    got_b = np.concatenate([rep['lo'], rep['hi'], rep['box_lo'], rep['box_hi']])
    assert np.array_equal(got_b, want_b)
    assert ids.dtype == torch.int32 and np.array_equal(_np(ids), want_ids)
    assert _same_bytes(_np(out), p[want_ids])


def test_crop_signs_zeros_and_repeats_at_the_rank():
    """a negative float's bit pattern orders backwards; +-0 are one value; the rank falls inside a run of equal values"""
    from points2surf_amd import prepare
    x = np.array([-2.0, -2.0, -0.0, 0.0, 0.0, -1.0, 3.0, -2.0, 3.0, -5.0, 1e-45, -1e-45, 7.5], np.float32)
    p = np.stack([x, np.roll(x, 3), -x], axis=1)
    n = len(x)
    for q in (0.09, 0.17, 0.26, 0.34, 0.42, 0.49):
        r_lo, r_hi = M.quantile_ranks(n, q)
        out, ids, rep = prepare.crop(p, q, 0.0, want_report=True)
        for a in range(3):
            s = np.sort(p[:, a])
            assert rep['lo'][a] == s[r_lo] and rep['hi'][a] == s[r_hi], (q, a)
        want_ids, want_b = M.crop(p, q, 0.0)
        assert np.array_equal(rep['box_lo'], want_b[6:9]) and np.array_equal(rep['box_hi'], want_b[9:12])
        assert np.array_equal(_np(ids), want_ids) and _same_bytes(_np(out), p[want_ids])


def test_crop_removes_a_far_return_and_off_is_the_identity():
    from points2surf_amd import prepare
    p = M.scan_like(2000, seed=1, outliers=0.0)
    p[17] = (250.0, -3.0, 0.1)
    p[3, 0] = -0.0
    out, ids = prepare.crop(p, 0.01, 1.0)
    assert np.array_equal(_np(ids), np.delete(np.arange(2000), 17))
    out, ids = prepare.crop(p, 0.0, 1.0)
    assert _same_bytes(_np(out), p) and np.array_equal(_np(ids), np.arange(2000))       # the sign of -0 included


# ---- statistical outliers -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _outlier_reference(n, k):
    p = M.seeded_cloud(n, seed=2)
    p.setflags(write=False)
    ids, info = M.remove_outliers(p, k, 2.0)
    return p, ids, info


@pytest.mark.parametrize('k', (4, 16))
@pytest.mark.parametrize('n', SIZES)
def test_outlier_statistic_mean_std_and_flags(n, k):
    from points2surf_amd import prepare
    p, want_ids, info = _outlier_reference(n, k)
    out, ids, rep = prepare.remove_outliers(p, k, 2.0, want_report=True)
    if n < 2:
        assert rep['d'] is None and np.array_equal(_np(ids), [0]) and _same_bytes(_np(out), p)
        return
    d, thr = info['d'], info['threshold']
    band = np.abs(d - thr) <= BAND * thr
    got = _np(rep['d'])
    if n == 2:
        # two points have one distance: d_0 = d_1 = mean = threshold exactly and std = 0, whatever the seed, so the band
        # cannot be empty; instead mean and std must be the model's very numbers, which makes every flag comparable
        assert band.all() and info['std'] == 0.0 and rep['std'] == 0.0 and rep['mean'] == info['mean'] and rep['threshold'] == thr
        band[:] = False
    assert not band.any()                            # on the model alone: the seeds leave the band empty
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), d.view(np.uint64))
    print('n', n, 'k', k, 'mean', rep['mean'], info['mean'], 'std', rep['std'], info['std'], 'threshold', rep['threshold'], thr)
    assert rep['k'] == min(k, n - 1)
    assert abs(rep['mean'] - info['mean']) <= 1e-12 * info['mean']
    assert abs(rep['std'] - info['std']) <= 1e-11 * info['std']
    keep = np.zeros(n, bool)
    keep[_np(ids)] = True
    assert np.array_equal(keep[~band], (d <= thr)[~band])
    assert np.array_equal(_np(ids), want_ids) and _same_bytes(_np(out), p[want_ids])


def test_outliers_hand_made():
    from points2surf_amd import prepare
    k = 6
    rng = np.random.default_rng(5)
    blob = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    # a cluster of k + 2 identical points: the k + 1 nearest of each are all at distance 0
    p = np.concatenate([np.repeat(np.array([[0.25, -0.5, 0.125]], np.float32), k + 2, 0), blob])
    out, ids, rep = prepare.remove_outliers(p, k, 2.0, want_report=True)
    d = _np(rep['d'])
    assert (d[:k + 2] == 0.0).all() and (d[k + 2:] > 0.0).all()
    assert np.array_equal(d.view(np.uint64), M.outlier_statistic(p, k).view(np.uint64))
    # all points equal: std = 0, everything is kept
    same = np.repeat(np.array([[1.5, 2.5, -3.5]], np.float32), 70, 0)
    out, ids, rep = prepare.remove_outliers(same, k, 2.0, want_report=True)
    assert rep['mean'] == 0.0 and rep['std'] == 0.0 and np.array_equal(_np(ids), np.arange(70)) and _same_bytes(_np(out), same)
    # one point at 1000 times the extent: d ~ 2000 against a mean of ~ 7 and a std of ~ 115 -- it goes and nothing else
    far = blob.copy()
    far[123] = (2000.0, 0.0, 0.0)
    out, ids = prepare.remove_outliers(far, k, 2.0)
    assert np.array_equal(_np(ids), np.delete(np.arange(300), 123))
    # n = k + 1: every neighbourhood is the whole cloud; k above n - 1 is clamped to the same
    few = blob[:k + 1]
    want = M.outlier_statistic(few, k)
    for kk in (k, 64):
        out, ids, rep = prepare.remove_outliers(few, kk, 2.0, want_report=True)
        assert rep['k'] == k and np.array_equal(_np(rep['d']).view(np.uint64), want.view(np.uint64))
        assert np.array_equal(_np(ids), M.remove_outliers(few, kk, 2.0)[0])
    # n = 1, and the stage switched off
    out, ids = prepare.remove_outliers(blob[:1], k, 2.0)
    assert np.array_equal(_np(ids), [0]) and _same_bytes(_np(out), blob[:1])
    out, ids = prepare.remove_outliers(far, k, 0.0)
    assert np.array_equal(_np(ids), np.arange(300)) and _same_bytes(_np(out), far)


# ---- voxel thinning -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', (17, 257, 4099))
def test_voxel_resolution_count_and_ids(n):
    from points2surf_amd import prepare
    p = M.seeded_cloud(n, seed=3)
    for budget in (1, 2, n // 3, n - 1):
        want_ids, want_R, want_occ = M.voxel_thin(p, budget)
        out, ids, rep = prepare.voxel_thin(p, budget, want_report=True)
        assert (rep['R'], rep['occupied']) == (want_R, want_occ), budget
        assert np.array_equal(_np(ids), want_ids) and _same_bytes(_np(out), p[want_ids])
        assert len(want_ids) <= budget
    out, ids, rep = prepare.voxel_thin(p, 1, want_report=True)
    assert rep['R'] == 1 and ids.shape[0] == 1       # one cell, one point
    for budget in (n, n + 5):                        # nothing to do: the input's bytes
        out, ids, rep = prepare.voxel_thin(p, budget, want_report=True)
        assert rep['R'] == 0 and _same_bytes(_np(out), p) and np.array_equal(_np(ids), np.arange(n))
    for R in (1, 7, 1024):                           # a given resolution
        want_ids, _, want_occ = M.voxel_thin(p, resolution=R)
        out, ids, rep = prepare.voxel_thin(p, resolution=R, want_report=True)
        assert (rep['R'], rep['occupied']) == (R, want_occ) and np.array_equal(_np(ids), want_ids)


def test_voxel_faces_clamping_and_mirror_pairs():
    from points2surf_amd import prepare
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    p = np.concatenate([corners, 0.25 + 0.5 * corners])          # the corners of the unit cube and the centres of R = 2
    out, ids, rep = prepare.voxel_thin(p, resolution=2, want_report=True)
    assert rep['occupied'] == 8 and np.array_equal(_np(ids), np.arange(8, 16))
    # 0.75 * 4 = 3 is a face: (0.75, 0.75, 0.75) lies in the last cell, where the corner (1, 1, 1) is clamped to -- 15 cells;
    # both are at the same distance from its centre 0.875, so the corner (id 7) stays and the inner point (id 15) goes
    out, ids, rep = prepare.voxel_thin(p, resolution=4, want_report=True)
    assert rep['occupied'] == 15 and np.array_equal(_np(ids), np.arange(15))
    out, ids, rep = prepare.voxel_thin(p, 8, want_report=True)
    assert rep['R'] == 3 and rep['occupied'] == 8 and np.array_equal(_np(ids), M.voxel_thin(p, 8)[0])
    # 0.5 is a face of R = 2 and belongs to the upper cell; 0.625 and 0.875 mirror each other about its centre 0.75
    q = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.25], [0.875, 0.25, 0.25], [0.625, 0.25, 0.25]], np.float32)
    out, ids = prepare.voxel_thin(q, resolution=2)
    assert np.array_equal(_np(ids), [0, 1, 3]) and _same_bytes(_np(out), q[[0, 1, 3]])
    # all points equal (extent 0): one cell
    same = np.repeat(np.array([[1.5, 2.5, -3.5]], np.float32), 9, 0)
    out, ids, rep = prepare.voxel_thin(same, 4, want_report=True)
    assert np.array_equal(_np(ids), [0]) and rep['occupied'] == 1


# ---- unit cube ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', (2, 17, 257, 4099))
def test_normalize_bytes_and_span(n):
    from points2surf_amd import prepare
    p = (M.seeded_cloud(n, seed=4).astype(np.float64) * 37.0 + np.array([120.0, -45.0, 8.0])).astype(np.float32)
    want, c, s = M.normalize(p)
    out, frame = prepare.normalize(p)
    assert out.dtype == torch.float32 and _same_bytes(_np(out), want)
    assert np.array_equal(frame['centre'], c) and frame['scale'] == s
    ext = p.max(0).astype(np.float64) - p.min(0).astype(np.float64)
    a = int(np.argmax(ext))
    got = _np(out)
    assert got[:, a].min() == -0.5 and got[:, a].max() == 0.5
    back = _np(prepare.restore(out, frame))
    assert back.dtype == np.float64 and np.array_equal(back, M.restore(want, c, s))
    assert np.abs(back - p.astype(np.float64)).max() <= 2.0 ** -24 * ext.max()


def test_normalize_flat_degenerate_and_engine():
    from points2surf_amd import engine, prepare
    p = M.seeded_cloud(257, seed=6)
    flat = p.copy()
    flat[:, 2] = 0.375
    out, frame = prepare.normalize(flat)
    assert _same_bytes(_np(out), M.normalize(flat)[0]) and (_np(out)[:, 2] == 0.0).all()
    with pytest.raises(prepare.Refused, match='extent 0'):
        prepare.normalize(np.repeat(p[:1], 5, 0))
    with pytest.raises(prepare.Refused, match='extent 0'):
        prepare.normalize(p[:1])
    out, _ = prepare.normalize(M.scan_like(4099, seed=3, outliers=0.0))
    cloud = engine.Cloud(out)
    try:
        q = cloud.query_grid(32, 3)
    finally:
        cloud.close()
    assert q.shape[0] > 0 and q.shape[1] == 3


# ---- the stages composed ------------------------------------------------------------------------------------------------

def _assert_band_empty(p, k):
    """on the model alone: no d_i of the cloud that reaches the outlier stage lies in the band around the threshold"""
    mid = M.finite_ids(p)
    mid = mid[M.crop(p[mid], 0.01, 1.0)[0]]
    info = M.remove_outliers(p[mid], k, 2.0)[1]
    assert not (np.abs(info['d'] - info['threshold']) <= BAND * info['threshold']).any()


@pytest.mark.parametrize('thin', ('random', 'voxel'))
def test_prepare_equals_the_models_composition(thin):
    from points2surf_amd import prepare
    p = M.scan_like(1200, seed=9, far=2)
    p[5] = np.nan
    p[77, 1] = np.inf
    opts = dict(max_points=500, thin=thin, k=8, seed=3)
    want, want_kept, (c, s), want_rep = M.prepare(p, **opts)
    # the outlier flags of the composition are exact only if no d_i lies in the band around the threshold
    _assert_band_empty(p, 8)
    out, kept, frame, rep = prepare.prepare(p, **opts)
    assert kept.dtype == torch.int32 and np.array_equal(_np(kept), want_kept)
    assert _same_bytes(_np(out), want)
    assert np.array_equal(frame['centre'], c) and frame['scale'] == s and frame['kept'] is kept
    for key in ('points_in', 'nonfinite', 'cropped', 'outliers', 'thinned', 'points_out', 'R'):
        assert rep[key] == want_rep[key], key
    assert rep['nonfinite'] == 2 and rep['cropped'] == 2 and rep['outliers'] > 0 and rep['points_out'] <= 500
    out2, kept2, frame2, rep2 = prepare.prepare(p, **opts)
    assert _same_bytes(_np(out2), _np(out)) and np.array_equal(_np(kept2), _np(kept)) and rep2 == rep
    assert frame2['scale'] == frame['scale'] and np.array_equal(frame2['centre'], frame['centre'])


def test_prepare_with_every_stage_off_is_the_standin_arithmetic():
    from points2surf_amd import prepare
    q = M.seeded_cloud(257, seed=8)
    out, kept, frame, rep = prepare.prepare(q, crop_quantile=0, std_ratio=0, max_points=0)
    # synth.standin_cloud: (p - (lo + hi) * 0.5) / ext in float64, rounded once -- with the division replaced by * (1 / ext)
    x = q.astype(np.float64)
    lo, hi = x.min(axis=0), x.max(axis=0)
    assert _same_bytes(_np(out), ((x - (lo + hi) * 0.5) * (1.0 / (hi - lo).max())).astype(np.float32))
    assert np.array_equal(_np(kept), np.arange(257))
    assert (rep['nonfinite'], rep['cropped'], rep['outliers'], rep['thinned'], rep['points_out']) == (0, 0, 0, 0, 257)
    out, kept, frame, rep = prepare.prepare(q, crop_quantile=0, std_ratio=0, max_points=257)
    assert rep['thinned'] == 0 and np.array_equal(_np(kept), np.arange(257))


# ---- command line -------------------------------------------------------------------------------------------------------

def _read_report(path):
    with open(path, newline='') as f:
        return {r['file']: r for r in csv.DictReader(f)}


def test_command_line(tmp_path, capsys):
    from points2surf_amd import ply, prepare
    raw, out = tmp_path / 'raw', tmp_path / 'dataset'
    raw.mkdir()
    a = M.scan_like(600, seed=21, outliers=0.0)
    a = (a.astype(np.float64) * 12.0 + np.array([30.0, -7.0, 2.0])).astype(np.float32)
    a[10] = np.nan
    a[20, 2] = np.inf
    a[30] = (5000.0, 4000.0, -3000.0)                # a far return
    ply.write_ply(str(raw / 'b_scan.ply'), a)                                            # vertices only
    b = M.scan_like(400, seed=22, outliers=0.0)
    np.savetxt(str(raw / 'a_scan.xyz'), np.concatenate([b, np.ones((400, 2))], axis=1))   # five columns: the first three count
    np.save(str(raw / 'few.npy'), M.seeded_cloud(5, seed=1))
    np.save(str(raw / 'same.npy'), np.repeat(np.array([[1.0, 2.0, 3.0]], np.float32), 40, 0))
    (raw / 'empty.txt').write_bytes(b'')
    (raw / 'notes.md').write_text('not a cloud')
    argv = ['--indir', str(raw), '--outdir', str(out), '--k', '8', '--max_points', '300', '--seed', '5']
    assert prepare.main(argv) == 0
    assert sorted(os.listdir(out / '04_pts')) == ['a_scan.xyz.npy', 'b_scan.xyz.npy']
    assert sorted(os.listdir(out / '04_pts_frame')) == ['a_scan.npz', 'b_scan.npz']
    assert (out / 'testset.txt').read_text() == 'a_scan\nb_scan\n'
    rep = _read_report(out / 'prepare_report.csv')
    assert sorted(rep) == ['a_scan.xyz', 'b_scan.ply', 'empty.txt', 'few.npy', 'same.npy']
    assert rep['empty.txt']['refused'].startswith('unreadable')
    assert rep['few.npy']['refused'].startswith('fewer than k + 1 = 9 points left') and rep['few.npy']['points_in'] == '5'
    assert rep['same.npy']['refused'] == 'extent 0'
    r = rep['b_scan.ply']
    assert (r['points_in'], r['nonfinite'], r['cropped'], r['points_out'], r['refused']) == ('600', '2', '1', '300', '')
    assert int(r['outliers']) + int(r['thinned']) == 600 - 2 - 1 - 300
    _assert_band_empty(a, 8)
    want, want_kept, (c, s), want_rep = M.prepare(a, k=8, max_points=300, seed=5)
    assert int(r['outliers']) == want_rep['outliers']
    got = np.load(out / '04_pts' / 'b_scan.xyz.npy')
    assert got.dtype == np.float32 and _same_bytes(got, want)
    with np.load(out / '04_pts_frame' / 'b_scan.npz') as z:
        assert z['kept'].dtype == np.int32 and np.array_equal(z['kept'], want_kept)
        assert z['centre'].dtype == np.float64 and np.array_equal(z['centre'], c) and float(z['scale']) == s
        frame = dict(centre=z['centre'].copy(), scale=float(z['scale']))
    assert float(r['scale']) == s and float(r['centre_x']) == c[0]
    r = rep['a_scan.xyz']
    assert (r['points_in'], r['nonfinite'], r['refused']) == ('400', '0', '') and int(r['points_out']) == 300
    # a second run skips what is up to date and leaves the files alone
    stamp = os.path.getmtime(out / '04_pts' / 'b_scan.xyz.npy')
    capsys.readouterr()
    assert prepare.main(argv) == 0
    text = capsys.readouterr().out
    assert 'up to date: a_scan.xyz' in text and 'up to date: b_scan.ply' in text
    assert os.path.getmtime(out / '04_pts' / 'b_scan.xyz.npy') == stamp
    assert _read_report(out / 'prepare_report.csv') == rep and (out / 'testset.txt').read_text() == 'a_scan\nb_scan\n'
    # restore: a hand-written mesh in the unit cube back into the scan's frame
    meshes, restored = tmp_path / 'meshes', tmp_path / 'restored'
    meshes.mkdir()
    v = np.array([[-0.5, -0.5, -0.5], [0.5, -0.25, 0.0], [0.0, 0.5, 0.125], [0.3, 0.1, -0.2]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]])
    ply.write_ply(str(meshes / 'b_scan.ply'), v, f)
    ply.write_ply(str(meshes / 'unknown.ply'), v, f)
    assert prepare.main(['--outdir', str(out), '--stage', 'restore', '--meshes', str(meshes), '--restored', str(restored)]) == 0
    assert os.listdir(restored) == ['b_scan.ply']
    rv, rf = ply.read_ply(str(restored / 'b_scan.ply'))
    want_v = v.astype(np.float64) / frame['scale'] + frame['centre']
    assert np.array_equal(np.asarray(rv, np.float32), want_v.astype(np.float32)) and np.array_equal(rf, f)
    assert np.array_equal(_np(prepare.restore(v, frame)), want_v)
