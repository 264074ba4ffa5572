"""``python -m points2surf_amd.baseline`` on a temporary data set made from one fixture mesh: 06_normals, the Poisson
reconstruction and its two reports, and the reconstruction's F-score against the model's (tests/poisson_model.py)."""
import csv
import os

import numpy as np
import pytest
import torch

import poisson_model as P
from test_mesh_sdf_model import MESHES, load

pytestmark = pytest.mark.gpu

DEPTH = 6


def test_stage_all_on_one_fixture_mesh(tmp_path):
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
    np.save(os.path.join(root, '04_pts', 'no_mesh.xyz.npy'), pts[:100])          # a cloud without a mesh: skipped with a note
    baseline.main(['--indir', root, '--stage', 'all', '--depth', str(DEPTH)])

    # 06_normals: the normal of the exactly nearest face
    nrm = np.load(os.path.join(root, '06_normals', stem + '.xyz.npy'))
    mesh = gt_sdf.TriMesh(v, f.astype(np.int32))
    try:
        face = mesh.distance(pts, signed=False, want_face=True)[1].cpu().numpy()
    finally:
        mesh.close()
    assert nrm.dtype == np.float32 and nrm.shape == (20000, 3)
    assert np.array_equal(nrm, baseline.face_normals(v, f)[face].astype(np.float32))
    assert not os.path.exists(os.path.join(root, '06_normals', 'no_mesh.xyz.npy'))

    # the reconstruction loads and is closed
    f_rec = os.path.join(root, '06_poisson_rec_gt_normals', stem + '.ply')
    rv, rf = ply.read_ply(f_rec)
    rec = gt_sdf.TriMesh(np.asarray(rv, np.float32), np.asarray(rf).astype(np.int32))
    try:
        assert rec.info()['closed'] and rf.shape[0] > 0
    finally:
        rec.close()

    # both reports: one row of finite numbers
    for report, first in (('comp_poisson_rec_gt_normals.csv', 2), ('quality_poisson_rec_gt_normals.csv', 2)):
        rows = list(csv.reader(open(os.path.join(root, report))))
        assert len(rows) == 2 and rows[1][0] == f_rec
        numbers = []
        for x in rows[1][first:]:
            try:
                numbers.append(float(x))             # the note column of the quality report is text
            except ValueError:
                pass
        assert len(numbers) >= 4 and np.isfinite(numbers).all()

    # F-score at tau = 2 h: at least the model's depth-6 volume through the same marching cubes, minus 0.01 (skipped for a
    # mesh on which the model itself scores below 0.5: the baseline, not the solver, fails there)
    chi, lev, _ = P.solve(pts, nrm, DEPTH)
    vol, _ = P.volume(lev, chi)
    mv, mf, _ = engine.marching_cubes(torch.from_numpy(vol).cuda(), model_space=False, fix_inversion=True)
    f_model = os.path.join(root, 'model.ply')
    ply.write_ply(f_model, (lev.lo + lev.h * mv.cpu().numpy().astype(np.float64)).astype(np.float32), mf.cpu().numpy())
    tau = 2.0 * lev.h
    f_ref = os.path.join(root, '03_meshes', name)
    key = 'fscore@%g' % tau
    got = metrics.mesh_quality(f_rec, f_ref, samples_per_model=20000, taus=(tau,), iou_res=32)[key]
    want = metrics.mesh_quality(f_model, f_ref, samples_per_model=20000, taus=(tau,), iou_res=32)[key]
    print(name, 'h', lev.h, 'F-score device', got, 'model', want)
    if want >= 0.5:
        assert got >= want - 0.01
