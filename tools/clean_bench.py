"""Timing of the mesh repair (points2surf_amd/clean.py: p2s_mesh_repair) on one device against two host baselines on the
same box: ``ply.merge_vertices`` (the weld alone) and the numpy model of the whole repair (tests/clean_model.py).  Meshes:
the soups of the three fixture meshes (every face its own vertices, a third flipped, 100 duplicate and 100 collapsed faces)
and the soup of the engine's own 256^3 iso-surface of the test shape.  The call synchronises its stream, so it is timed on the
host clock around a device that is idle before it: two warm-up calls, then ``--reps`` calls; median, minimum and maximum.
One JSON line per mesh.
    python tools/clean_bench.py [--skip-large] [--skip-model-large] [--reps N]"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
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
    ap.add_argument('--skip-model-large', action='store_true', help='no numpy-model baseline for the 0.92 M-face mesh (minutes)')
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    import torch
    import clean_model
    from points2surf_amd import clean, engine, ply, synth
    meshes = []
    for f in sorted(glob.glob(os.path.join(FIX, '03_meshes', '*.ply'))):
        v, fc = ply.read_ply(f)
        meshes.append((os.path.basename(f)[:8], np.asarray(v, np.float32), fc))
    if not args.skip_large:
        cloud = engine.Cloud(np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy')))
        w, cfg = synth.make_weights('p2s_max')
        sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), 256, 3)
        vol, _ = engine.sdf_volume(q, sdf, 256, 5, 13.0, clamp=True)
        v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
        meshes.append(('engine256', v.cpu().numpy().astype(np.float32), f.cpu().numpy()))
    for name, v, f in meshes:
        large = name == 'engine256'
        sv, sf, _ = clean_model.soup(v, f, seed=1)
        vt, ft = torch.from_numpy(sv).cuda(), torch.from_numpy(sf).cuda()
        rep = clean.repair(vt, ft)[3]
        row = dict(mesh=name, soup_verts=len(sv), soup_faces=len(sf), report=rep)
        row['device_repair'] = timed(lambda: clean.repair(vt, ft), args.reps)
        t = time.perf_counter()
        ply.merge_vertices(sv, sf)
        row['host_merge_vertices_ms'] = (time.perf_counter() - t) * 1e3
        if not (large and args.skip_model_large):
            t = time.perf_counter()
            want = clean_model.repair(sv, sf)
            row['host_model_repair_ms'] = (time.perf_counter() - t) * 1e3
            row['model_report_equal'] = want[3] == rep
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
