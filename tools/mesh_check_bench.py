"""Timing of the self-intersection check (TriMesh.check: p2s_mesh_check) on one device: the walk of the octree against
the exhaustive kernel on the same box, for the three fixture meshes and the engine's own 256^3 iso-surface of the test
shape.  The call synchronises its stream, so it is timed on the host clock around a device that is idle before it: two
warm-up calls, then ``--reps`` calls; median, minimum and maximum.  On the large mesh the exhaustive kernel runs once,
without a warm-up.  Reports only (no pairs are stored).  One JSON line per mesh.
    python tools/mesh_check_bench.py [--skip-large] [--reps N]"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FIX = os.path.join(REPO, 'tests', 'golden', 'abc_minimal')


def timed(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-large', action='store_true')
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    from points2surf_amd import engine, gt_sdf, ply, synth
    meshes = []
    for f in sorted(glob.glob(os.path.join(FIX, '03_meshes', '*.ply'))):
        v, fc = ply.read_ply(f)
        meshes.append((os.path.basename(f)[:8], np.asarray(v, np.float32), np.asarray(fc, np.int32)))
    if not args.skip_large:
        cloud = engine.Cloud(np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy')))
        w, cfg = synth.make_weights('p2s_max')
        sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), 256, 3)
        vol, _ = engine.sdf_volume(q, sdf, 256, 5, 13.0, clamp=True)
        v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
        meshes.append(('engine256', v.cpu().numpy().astype(np.float32), f.cpu().numpy().astype(np.int32)))
    for name, v, f in meshes:
        large = name == 'engine256'
        mesh = gt_sdf.TriMesh(v, f)
        try:
            rep = mesh.check()
            row = dict(mesh=name, verts=len(v), faces=len(f), grid=mesh.info()['grid'], report=rep,
                       candidates_per_face=rep['candidates'] / max(rep['faces_tested'], 1))
            row['index'] = timed(lambda: mesh.check(), args.reps)
            row['exhaustive'] = timed(lambda: mesh.check(method='exhaustive'), 1 if large else args.reps, warm=0 if large else 2)
            ex = mesh.check(method='exhaustive') if not large else None
            if ex is not None:
                row['exhaustive_candidates'] = ex['candidates']
                row['reports_equal'] = all(ex[k] == rep[k] for k in rep if k != 'candidates')
        finally:
            mesh.close()
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
