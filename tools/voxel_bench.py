"""Timing of the voxelisation (TriMesh.voxelize: p2s_mesh_voxelize) on one device: the walk of the octree against the
exhaustive kernel at ``--res`` (128) on the largest fixture mesh and on the engine's own 256^3 iso-surface of the test
shape, welded by the repair (the raw iso-surface repeats vertices under different indices and is not closed).  The call
synchronises its stream, so it is timed on the host clock around a device that is idle before it: two warm-up calls, then
``--reps`` calls; median, minimum and maximum.  On the large mesh the exhaustive kernel runs once, without a warm-up.
A mesh that is still not closed after the repair is reported as such and not timed (no occupancy is defined for it).
One JSON line per mesh.
    python tools/voxel_bench.py [--skip-large] [--reps N] [--res R]"""
import argparse
import glob
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
FIX = os.path.join(REPO, 'tests', 'golden', 'abc_minimal')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-large', action='store_true')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=128)
    args = ap.parse_args()
    from mesh_check_bench import timed
    from points2surf_amd import clean, engine, gt_sdf, ply, synth
    files = sorted(glob.glob(os.path.join(FIX, '03_meshes', '*.ply')), key=os.path.getsize)
    v, fc = ply.read_ply(files[-1])
    meshes = [(os.path.basename(files[-1])[:8], np.asarray(v, np.float32), np.asarray(fc, np.int32), None)]
    if not args.skip_large:
        cloud = engine.Cloud(np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy')))
        w, cfg = synth.make_weights('p2s_max')
        sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), 256, 3)
        vol, _ = engine.sdf_volume(q, sdf, 256, 5, 13.0, clamp=True)
        v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
        v, f, _, rep = clean.repair(v, f)
        meshes.append(('engine256', v.cpu().numpy().astype(np.float32), f.cpu().numpy().astype(np.int32), rep))
    for name, v, f, repair in meshes:
        large = name == 'engine256'
        mesh = gt_sdf.TriMesh(v, f)
        try:
            info = mesh.info()
            row = dict(mesh=name, verts=len(v), faces=len(f), res=args.res, closed=info['closed'], components=info['components'],
                       bad_edges=info['bad_edges'], octree_cells_per_axis=info['grid'])
            if repair is not None:
                row['repair'] = dict((k, repair[k]) for k in ('welded', 'holes_filled', 'holes_left', 'verdict') if k in repair)
            if info['closed']:
                cap = args.res ** 3                           # a measurement: every undecided voxel is taken
                _, rep = mesh.voxelize(args.res, max_fallback=cap, want_report=True)
                row['report'] = rep
                row['index'] = timed(lambda: mesh.voxelize(args.res, max_fallback=cap), args.reps)
                row['exhaustive'] = timed(lambda: mesh.voxelize(args.res, method='exhaustive', max_fallback=cap),
                                          1 if large else args.reps, warm=0 if large else 2)
                _, ex = mesh.voxelize(args.res, method='exhaustive', max_fallback=cap, want_report=True)
                row['exhaustive_tests'] = ex['tests']
                row['reports_equal'] = all(ex[k] == rep[k] for k in rep if k != 'tests')
        finally:
            mesh.close()
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
