"""The Screened Poisson baseline of the reference's ``eval_dataset.py`` on the device: the ground-truth normal of every
cloud point (``06_normals``), the reconstruction from them (``06_poisson_rec_gt_normals``, points2surf_amd.poisson in the
place of ``meshlabserver`` + ``poisson.mlx``) and its reports next to the network's.

``python -m points2surf_amd.baseline --indir DATASET [--stage normals|poisson|compare|all] [--depth 8] [--point_weight 4]
[--scale 1.1] [--dataset FILE] [--normals gt|estimated] [--k 16]``

``--normals gt``: the normal of a point is that of the EXACTLY nearest face of ``03_meshes/<stem>.ply``
(TriMesh.distance(want_face=True)); the reference's ``utils.get_pts_normals`` takes the nearest of 100,000 surface samples
instead.  A cloud without a mesh is skipped with a note.

``--normals estimated``: the reference's ``06_poisson_rec`` variant (``normals_poisson.mlx``), from the cloud alone
(points2surf_amd.normals: PCA over the ``--k`` nearest points, oriented along the minimum spanning forest): ``06_normals_est``
for EVERY ``04_pts`` cloud -- no mesh is needed, so a ``real_world`` set works --, ``06_poisson_rec``,
``comp_poisson_rec.csv`` / ``quality_poisson_rec.csv`` where ``03_meshes`` exists, and ``normals_est_report.csv`` for the
shapes that have ``06_normals`` as well.
"""
import argparse
import csv
import os
import tempfile

import numpy as np

from . import gt_sdf as _gt
from . import metrics as _metrics
from . import normals as _normals
from . import ply as _ply
from . import poisson as _poisson
from .file_utils import call_necessary as _call_necessary

STAGES = ('normals', 'poisson', 'compare', 'all')
REC_DIR = '06_poisson_rec_gt_normals'
# --normals -> (directory of the normals, directory of the reconstructions = the suffix of the reports)
VARIANTS = {'gt': ('06_normals', REC_DIR), 'estimated': ('06_normals_est', '06_poisson_rec')}
EST_REPORT = 'normals_est_report.csv'


def _stems(indir, need_mesh=True):
    """(stem, cloud file, mesh file) of every 04_pts cloud, in name order; clouds without a 03_meshes mesh are noted and left out"""
    pts_dir, mesh_dir = os.path.join(indir, '04_pts'), os.path.join(indir, '03_meshes')
    out = []
    for name in sorted(f for f in os.listdir(pts_dir) if f.endswith('.xyz.npy')):
        stem = name[:-len('.xyz.npy')]
        mesh = os.path.join(mesh_dir, stem + '.ply')
        if need_mesh and not os.path.isfile(mesh):
            print('%s: no mesh in 03_meshes, skipped' % name)
            continue
        out.append((stem, os.path.join(pts_dir, name), mesh))
    return out


def face_normals(verts, faces):
    """unit normals [F, 3] float64 of the faces (0 for a face without area)"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.divide(n, length, out=np.zeros_like(n), where=length > 0)


def point_normals(verts, faces, points, device=None):
    """float32 [N, 3]: for every point the unit normal of its nearest face"""
    mesh = _gt.TriMesh(np.asarray(verts, np.float32), np.asarray(faces), device=device)
    try:
        _, face = mesh.distance(np.asarray(points, np.float32), signed=False, want_face=True)
    finally:
        mesh.close()
    return face_normals(verts, faces)[face.cpu().numpy().astype(np.int64)].astype(np.float32)


def write_normals(indir, device=None):
    """06_normals/<stem>.xyz.npy for every 04_pts cloud that has a 03_meshes mesh; returns the files written"""
    out_dir = os.path.join(indir, '06_normals')
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for stem, f_pts, f_mesh in _stems(indir):
        f_out = os.path.join(out_dir, stem + '.xyz.npy')
        if not _call_necessary([f_pts, f_mesh], [f_out]):
            continue
        v, f = _ply.read_ply(f_mesh)
        np.save(f_out, point_normals(v, f, np.load(f_pts), device=device))
        written.append(f_out)
    return written


def normals_error(est, truth):
    """(mean unoriented angle between the two fields in degrees, share of the points with est . truth < 0); points where
    either normal is zero count in neither"""
    a, b = np.asarray(est, np.float64), np.asarray(truth, np.float64)
    la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    ok = (la > 0) & (lb > 0)
    if not ok.any():
        return float('nan'), float('nan')
    dot = (a[ok] * b[ok]).sum(axis=1) / (la[ok] * lb[ok])
    return float(np.degrees(np.arccos(np.minimum(np.abs(dot), 1.0))).mean()), float((dot < 0).mean())


def write_estimated_normals(indir, k=16, device=None):
    """06_normals_est/<stem>.xyz.npy for every 04_pts cloud (no mesh needed), and one row of normals_est_report.csv for
    every shape that has 06_normals too: shape, mean unoriented angle error in degrees, share of points whose estimate
    points against the ground truth, components, points, k; returns the files written"""
    out_dir = os.path.join(indir, VARIANTS['estimated'][0])
    os.makedirs(out_dir, exist_ok=True)
    written, rows = [], []
    for stem, f_pts, _ in _stems(indir, need_mesh=False):
        f_out = os.path.join(out_dir, stem + '.xyz.npy')
        f_gt = os.path.join(indir, VARIANTS['gt'][0], stem + '.xyz.npy')
        # a shape with ground truth is always made again: its report row needs the component count of this run
        if not os.path.isfile(f_gt) and not _call_necessary([f_pts], [f_out]):
            continue
        pts = np.load(f_pts).astype(np.float32)[:, :3]
        if pts.shape[0] < max(int(k), 4):
            print('%s: %d points < k = %d, skipped' % (stem, pts.shape[0], k))
            continue
        nrm, _, rep = _normals.estimate(pts, k=k, orient='mst', want_report=True, device=device)
        nrm = nrm.cpu().numpy()
        np.save(f_out, nrm)
        written.append(f_out)
        if os.path.isfile(f_gt):
            angle, against = normals_error(nrm, np.load(f_gt))
            rows.append([stem, '%.6f' % angle, '%.6f' % against, rep['components'], pts.shape[0], int(k)])
    if rows:
        f_rep = os.path.join(indir, EST_REPORT)
        with open(f_rep, 'w', newline='') as fh:
            out = csv.writer(fh)
            out.writerow(['shape', 'mean_angle_error_deg', 'share_against_gt', 'components', 'points', 'k'])
            out.writerows(rows)
        written.append(f_rep)
    return written


def write_reconstructions(indir, depth=8, point_weight=4.0, scale=1.1, device=None, normals='gt'):
    """06_poisson_rec_gt_normals/<stem>.ply from 04_pts and 06_normals (``normals='estimated'``: 06_poisson_rec from
    06_normals_est); returns [(file, report)]"""
    nrm_dir, rec_dir = VARIANTS[normals]
    out_dir = os.path.join(indir, rec_dir)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for stem, f_pts, _ in _stems(indir, need_mesh=False):
        f_nrm = os.path.join(indir, nrm_dir, stem + '.xyz.npy')
        f_out = os.path.join(out_dir, stem + '.ply')
        if not os.path.isfile(f_nrm):
            print('%s: no normals in %s, skipped' % (stem, nrm_dir))
            continue
        if not _call_necessary([f_pts, f_nrm], [f_out]):
            continue
        verts, faces, report = _poisson.reconstruct(np.load(f_pts).astype(np.float32), np.load(f_nrm).astype(np.float32), depth=depth,
                                                    point_weight=point_weight, scale=scale, want_report=True, device=device)
        _ply.write_ply(f_out, verts.cpu().numpy(), faces.cpu().numpy())
        written.append((f_out, report))
    return written


def compare(indir, dataset=None, normals='gt'):
    """comp_poisson_rec_gt_normals.csv (metrics.mesh_comparison, the reference's format, 10,000 samples) and
    quality_poisson_rec_gt_normals.csv (metrics.quality_comparison) for the shapes of ``dataset`` (default: valset.txt when
    it exists, else every reconstruction); returns the two files.  ``normals='estimated'``: comp_poisson_rec.csv and
    quality_poisson_rec.csv of 06_poisson_rec; a set without 03_meshes has nothing to compare against: a note, no files"""
    rec_dir = VARIANTS[normals][1]
    rec, ref = os.path.join(indir, rec_dir), os.path.join(indir, '03_meshes')
    if normals == 'estimated' and not os.path.isdir(ref):
        print('%s: no 03_meshes, nothing to compare %s against' % (indir, rec_dir))
        return ()
    if dataset is None and os.path.isfile(os.path.join(indir, 'valset.txt')):
        dataset = os.path.join(indir, 'valset.txt')
    f_comp = os.path.join(indir, 'comp_%s.csv' % rec_dir[len('06_'):])
    f_qual = os.path.join(indir, 'quality_%s.csv' % rec_dir[len('06_'):])
    listed = None
    if dataset is None:
        # the pairing rules match a reconstruction to the set by its stem, and without a list the set holds file names:
        # name every reconstruction instead
        listed = tempfile.NamedTemporaryFile('w', suffix='.txt', delete=False)
        listed.write('\n'.join(sorted(f.split('.')[0] for f in os.listdir(rec) if os.path.isfile(os.path.join(rec, f)))))
        listed.close()
        dataset = listed.name
    try:
        _metrics.mesh_comparison(rec, ref, 1, f_comp, samples_per_model=10000, dataset_file_abs=dataset)
        _metrics.quality_comparison(rec, ref, f_qual, dataset_file_abs=dataset)
    finally:
        if listed is not None:
            os.unlink(listed.name)
    return f_comp, f_qual


def main(argv=None):
    ap = argparse.ArgumentParser(description='the Screened Poisson baseline of a data set: 06_normals, 06_poisson_rec_gt_normals, reports (--normals estimated: 06_normals_est, 06_poisson_rec)')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--stage', choices=STAGES, default='all')
    ap.add_argument('--depth', type=int, default=8, help='finest level: 2^depth + 1 nodes per axis (3..9)')
    ap.add_argument('--point_weight', type=float, default=4.0)
    ap.add_argument('--scale', type=float, default=1.1)
    ap.add_argument('--dataset', default=None, help='file with the names of the shapes to compare (default: valset.txt)')
    ap.add_argument('--normals', choices=sorted(VARIANTS), default='gt',
                    help='gt: 06_normals from 03_meshes; estimated: 06_normals_est from the cloud alone -> 06_poisson_rec')
    ap.add_argument('--k', type=int, default=16, help='--normals estimated: neighbours of the PCA and of the orientation graph (4..64)')
    opt = ap.parse_args(argv)
    if opt.stage in ('normals', 'all'):
        for f in (write_normals(opt.indir) if opt.normals == 'gt' else write_estimated_normals(opt.indir, opt.k)):
            print(f)
    if opt.stage in ('poisson', 'all'):
        for f, rep in write_reconstructions(opt.indir, opt.depth, opt.point_weight, opt.scale, normals=opt.normals):
            print('%s  iterations %s  ms %.1f' % (f, [lv['iterations'] for lv in rep['levels']], sum(lv['ms'] for lv in rep['levels'])))
    if opt.stage in ('compare', 'all'):
        for f in compare(opt.indir, opt.dataset, normals=opt.normals):
            print(f)


if __name__ == '__main__':
    main()
