"""Timing of the scan path (points2surf_amd/scan.py): the time-of-flight scan set of each fixture mesh (its own poses, 176 x 144
rays per scan) and of the engine's own 256^3 mesh, indexed next to exhaustive, plus the 2,000 query points.  HIP events, one
warm-up, median of three; one JSON line per case, appended to profiles/scan/scan_bench.jsonl with --record.
    python tools/scan_bench.py [--skip-large] [--no-exhaustive-large] [--record]"""
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
    ap.add_argument('--no-exhaustive-large', action='store_true', help='skip the scan set x 0.92 M faces exhaustively')
    ap.add_argument('--record', action='store_true', help='append the rows to profiles/scan/scan_bench.jsonl')
    args = ap.parse_args()
    import torch
    from gt_sdf_bench import timed
    from points2surf_amd import engine, ply, scan, synth
    meshes = [(os.path.basename(f),) + tuple(ply.read_ply(f)) for f in sorted(glob.glob(os.path.join(FIX, '03_meshes', '*.ply')))]
    if not args.skip_large:
        pts = np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy'))
        w, cfg = synth.make_weights('p2s_max')
        sdf, q = engine.infer_shape(engine.Model(w, cfg), engine.Cloud(pts), engine.Rng(40938661), 256, 3)
        vol, _ = engine.sdf_volume(q, sdf, 256, 5, 13.0, clamp=True)
        v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
        meshes.append(('engine256.ply',) + ply.merge_vertices(v.cpu().numpy(), f.cpu().numpy()))
    rows = []
    for name, v, f in meshes:
        mesh = scan.TriMesh(np.asarray(v, np.float32), np.asarray(f))
        info = mesh.info()
        poses = scan.scan_poses(name)
        poses['noise'] = torch.from_numpy(poses['noise']).cuda()
        rays = poses['n_scans'] * 176 * 144
        row = dict(mesh=name[:8] if name[0] == '0' else name[:-4], faces=info['n_faces'], grid=info['grid'], scans=poses['n_scans'], rays=rays)
        res = scan.tof_scan(mesh, poses)
        row['hits'] = int(res['points'].shape[0])
        row['tests_per_ray'] = res['tests'] / rays
        row['index_ms'] = timed(lambda: scan.tof_scan(mesh, poses, method='index'))
        row['index_mrays_per_s'] = rays / row['index_ms'] / 1e3
        if not (name.startswith('engine256') and args.no_exhaustive_large):
            row['exhaustive_ms'] = timed(lambda: scan.tof_scan(mesh, poses, method='exhaustive'), reps=1 if name.startswith('engine256') else 3)
            row['exhaustive_mrays_per_s'] = rays / row['exhaustive_ms'] / 1e3
        if info['closed']:
            seed = scan.filename_to_hash(name)
            row['query_pts_ms'] = timed(lambda: scan.query_points(mesh, seed, 2000, 4.0 / 256))
        print(json.dumps(row), flush=True)
        rows.append(row)
        mesh.close()
    if args.record:
        out = os.path.join(REPO, 'profiles', 'scan')
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'scan_bench.jsonl'), 'a') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
