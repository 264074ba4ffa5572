"""The Screened Poisson baseline of the reference's ``eval_dataset.py`` on the device: the ground-truth normal of every
cloud point (``06_normals``), the reconstruction from them (``06_poisson_rec_gt_normals``, points2surf_amd.poisson in the
place of ``meshlabserver`` + ``poisson.mlx``) and its reports next to the network's.

``python -m points2surf_amd.baseline --indir DATASET [--stage normals|poisson|compare|all] [--depth 8] [--point_weight 4]
[--scale 1.1] [--dataset FILE]``

The normal of a point is that of the EXACTLY nearest face of ``03_meshes/<stem>.ply`` (TriMesh.distance(want_face=True));
the reference's ``utils.get_pts_normals`` takes the nearest of 100,000 surface samples instead.  A cloud without a mesh is
skipped with a note.
"""
import argparse
import os
import tempfile

import numpy as np

from . import gt_sdf as _gt
from . import metrics as _metrics
from . import ply as _ply
from . import poisson as _poisson
from .file_utils import call_necessary as _call_necessary

STAGES = ('normals', 'poisson', 'compare', 'all')
REC_DIR = '06_poisson_rec_gt_normals'


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


def write_reconstructions(indir, depth=8, point_weight=4.0, scale=1.1, device=None):
    """06_poisson_rec_gt_normals/<stem>.ply from 04_pts and 06_normals; returns [(file, report)]"""
    out_dir = os.path.join(indir, REC_DIR)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for stem, f_pts, _ in _stems(indir, need_mesh=False):
        f_nrm = os.path.join(indir, '06_normals', stem + '.xyz.npy')
        f_out = os.path.join(out_dir, stem + '.ply')
        if not os.path.isfile(f_nrm):
            print('%s: no normals in 06_normals, skipped' % stem)
            continue
        if not _call_necessary([f_pts, f_nrm], [f_out]):
            continue
        verts, faces, report = _poisson.reconstruct(np.load(f_pts).astype(np.float32), np.load(f_nrm).astype(np.float32), depth=depth,
                                                    point_weight=point_weight, scale=scale, want_report=True, device=device)
        _ply.write_ply(f_out, verts.cpu().numpy(), faces.cpu().numpy())
        written.append((f_out, report))
    return written


def compare(indir, dataset=None):
    """comp_poisson_rec_gt_normals.csv (metrics.mesh_comparison, the reference's format, 10,000 samples) and
    quality_poisson_rec_gt_normals.csv (metrics.quality_comparison) for the shapes of ``dataset`` (default: valset.txt when
    it exists, else every reconstruction); returns the two files"""
    rec, ref = os.path.join(indir, REC_DIR), os.path.join(indir, '03_meshes')
    if dataset is None and os.path.isfile(os.path.join(indir, 'valset.txt')):
        dataset = os.path.join(indir, 'valset.txt')
    f_comp = os.path.join(indir, 'comp_poisson_rec_gt_normals.csv')
    f_qual = os.path.join(indir, 'quality_poisson_rec_gt_normals.csv')
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
    ap = argparse.ArgumentParser(description='the Screened Poisson baseline of a data set: 06_normals, 06_poisson_rec_gt_normals, reports')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--stage', choices=STAGES, default='all')
    ap.add_argument('--depth', type=int, default=8, help='finest level: 2^depth + 1 nodes per axis (3..9)')
    ap.add_argument('--point_weight', type=float, default=4.0)
    ap.add_argument('--scale', type=float, default=1.1)
    ap.add_argument('--dataset', default=None, help='file with the names of the shapes to compare (default: valset.txt)')
    opt = ap.parse_args(argv)
    if opt.stage in ('normals', 'all'):
        for f in write_normals(opt.indir):
            print(f)
    if opt.stage in ('poisson', 'all'):
        for f, rep in write_reconstructions(opt.indir, opt.depth, opt.point_weight, opt.scale):
            print('%s  iterations %s  ms %.1f' % (f, [lv['iterations'] for lv in rep['levels']], sum(lv['ms'] for lv in rep['levels'])))
    if opt.stage in ('compare', 'all'):
        for f in compare(opt.indir, opt.dataset):
            print(f)


if __name__ == '__main__':
    main()
