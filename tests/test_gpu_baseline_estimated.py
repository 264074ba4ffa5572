"""``python -m points2surf_amd.baseline --normals estimated`` on a temporary data set made from one fixture mesh: 06_normals_est,
06_poisson_rec, its two reports and normals_est_report.csv, the F-score against the reconstruction from ground-truth normals
of the same run; and on a set that holds 04_pts alone (the reference's real_world)."""
import csv
import os

import numpy as np
import pytest
import torch

import normals_model as M
from test_mesh_sdf_model import MESHES, load

pytestmark = pytest.mark.gpu

DEPTH = 6
# F-score (tau = 2 h, depth 6, 20,000 samples) of the reconstruction from estimated normals may fall below that from
# ground-truth normals by what was measured once on this mesh -- MEASURED, see DESIGN 4.8 f11 -- plus 0.02 for sampling noise
MEASURED = 0.002679
MARGIN = MEASURED + 0.02


def _numbers(row, first):
    out = []
    for x in row[first:]:
        try:
            out.append(float(x))                         # the note column of the quality report is text
        except ValueError:
            pass
    return out


def test_estimated_normals_next_to_ground_truth(tmp_path, capsys):
    from points2surf_amd import baseline, engine, gt_sdf, metrics, ply
    name = MESHES[0]
    stem = name[:-len('.ply')]
    v, f = load(name)[:2]
    root = str(tmp_path)
    for d in ('03_meshes', '04_pts'):
        os.makedirs(os.path.join(root, d))
    ply.write_ply(os.path.join(root, '03_meshes', name), v, f.astype(np.int32))
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f.astype(np.int32)).cuda()
    pts = metrics.sample_surface(vt, ft, 20000, engine.Rng(3))[0].cpu().numpy()
    np.save(os.path.join(root, '04_pts', stem + '.xyz.npy'), pts)
    baseline.main(['--indir', root, '--normals', 'gt', '--stage', 'normals'])
    baseline.main(['--indir', root, '--normals', 'estimated', '--stage', 'all', '--depth', str(DEPTH)])

    gt = np.load(os.path.join(root, '06_normals', stem + '.xyz.npy'))
    est = np.load(os.path.join(root, '06_normals_est', stem + '.xyz.npy'))
    assert est.dtype == np.float32 and est.shape == (20000, 3) and np.isfinite(est).all()
    assert (np.abs(np.linalg.norm(est.astype(np.float64), axis=1) - 1.0) <= 2.0 ** -22).all()

    # the reconstruction loads and is closed; nothing of the gt variant was made by the estimated one
    f_rec = os.path.join(root, '06_poisson_rec', stem + '.ply')
    rv, rf = ply.read_ply(f_rec)
    rec = gt_sdf.TriMesh(np.asarray(rv, np.float32), np.asarray(rf).astype(np.int32))
    try:
        assert rec.info()['closed'] and rf.shape[0] > 0
    finally:
        rec.close()
    assert not os.path.exists(os.path.join(root, '06_poisson_rec_gt_normals'))
    assert not os.path.exists(os.path.join(root, 'comp_poisson_rec_gt_normals.csv'))

    for report in ('comp_poisson_rec.csv', 'quality_poisson_rec.csv'):
        rows = list(csv.reader(open(os.path.join(root, report))))
        assert len(rows) == 2 and rows[1][0] == f_rec
        numbers = _numbers(rows[1], 2)
        assert len(numbers) >= 4 and np.isfinite(numbers).all()
    rows = list(csv.reader(open(os.path.join(root, baseline.EST_REPORT))))
    assert len(rows) == 2 and rows[1][0] == stem
    angle, against, components, points, k = _numbers(rows[1], 1)
    assert np.isfinite([angle, against]).all() and 0.0 <= angle <= 90.0 and 0.0 <= against <= 1.0
    assert components >= 1 and points == 20000 and k == 16
    assert (angle, against) == tuple(float('%.6f' % x) for x in baseline.normals_error(est, gt))

    # F-score at tau = 2 h against the reconstruction from the ground-truth normals
    (f_gt, rep), = baseline.write_reconstructions(root, depth=DEPTH)
    tau = 2.0 * rep['h']
    f_ref = os.path.join(root, '03_meshes', name)
    key = 'fscore@%g' % tau
    got = metrics.mesh_quality(f_rec, f_ref, samples_per_model=20000, taus=(tau,), iou_res=32)[key]
    want = metrics.mesh_quality(f_gt, f_ref, samples_per_model=20000, taus=(tau,), iou_res=32)[key]
    # where Hoppe's rule itself, in the float64 model, leaves more than 1 % of this cloud misoriented, the rule and not the
    # kernel fails, and the comparison says nothing
    model = M.oriented(pts, 16, tree=True)[0]
    wrong = float(((model.astype(np.float64) * gt).sum(axis=1) < 0).mean())
    with capsys.disabled():
        print('\n%s: h %g, F-score estimated %.6f, ground truth %.6f, difference %.6f; angle error %.3f deg, against gt %.4f '
              '(model %.4f), components %d' % (name, rep['h'], got, want, want - got, angle, against, wrong, components))
    if wrong <= 0.01:
        assert got >= want - MARGIN
    else:
        print('%s: the model leaves %.2f %% of the points misoriented: F-score not compared' % (name, 100.0 * wrong))


def test_a_set_with_points_alone(tmp_path, capsys):
    from points2surf_amd import baseline, ply
    pts = M.torus()[0]
    root = str(tmp_path)
    os.makedirs(os.path.join(root, '04_pts'))
    np.save(os.path.join(root, '04_pts', 'scan.xyz.npy'), pts)
    baseline.main(['--indir', root, '--normals', 'estimated', '--stage', 'all', '--depth', '5', '--k', '12'])
    said = capsys.readouterr().out
    nrm = np.load(os.path.join(root, '06_normals_est', 'scan.xyz.npy'))
    assert nrm.shape == pts.shape and ((nrm.astype(np.float64) * M.torus()[1]).sum(axis=1) > 0).all()
    rv, rf = ply.read_ply(os.path.join(root, '06_poisson_rec', 'scan.ply'))
    assert len(rv) > 0 and len(rf) > 0
    assert 'no 03_meshes, nothing to compare' in said
    assert sorted(os.listdir(root)) == ['04_pts', '06_normals_est', '06_poisson_rec']          # no report of any kind
