"""Timing of the Screened Poisson baseline (points2surf_amd.poisson.reconstruct: p2s_poisson_reconstruct) on one device,
on a fixture cloud (``--stem``; default the largest, 86,648 points) with the normals of its mesh's nearest faces: one warm-up call, then ``--reps`` calls at
``--depth`` (8).  Per level the iterations, the milliseconds (device events around the level: its sorts, its system and
its CG) and milliseconds per CG iteration of the call with the median total; the whole call on the host clock.  One JSON
line.
    python tools/poisson_bench.py [--depth D] [--reps N] [--stem NAME]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FIX = os.path.join(REPO, 'tests', 'golden', 'abc_minimal')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stem', default=None, help='shape of tests/golden/abc_minimal (default: the one with the largest cloud)')
    args = ap.parse_args()
    import torch
    from points2surf_amd import baseline, ply, poisson
    stems = sorted(f[:-len('.xyz.npy')] for f in os.listdir(os.path.join(FIX, '04_pts')) if f.endswith('.xyz.npy'))
    stem = args.stem or max(stems, key=lambda t: os.path.getsize(os.path.join(FIX, '04_pts', t + '.xyz.npy')))
    pts = np.load(os.path.join(FIX, '04_pts', stem + '.xyz.npy')).astype(np.float32)
    v, f = ply.read_ply(os.path.join(FIX, '03_meshes', stem + '.ply'))
    nrm = baseline.point_normals(v, f, pts)
    runs = []
    for k in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts, faces, rep = poisson.reconstruct(pts, nrm, depth=args.depth, want_report=True)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0, rep, int(verts.shape[0]), int(faces.shape[0])))
    runs = sorted(runs[1:], key=lambda r: r[0])
    wall, rep, nv, nf = runs[len(runs) // 2]
    print(json.dumps(dict(shape=stem, points=int(pts.shape[0]), depth=args.depth, call_ms_median=1e3 * wall, call_ms_min=1e3 * runs[0][0],
                          call_ms_max=1e3 * runs[-1][0], verts=nv, faces=nf, h=rep['h'],
                          levels=[dict(depth=lv['depth'], n_occ=lv['n_occ'], iterations=lv['iterations'], residual=lv['residual'],
                                       ms=lv['ms'], ms_per_iteration=lv['ms'] / max(lv['iterations'], 1)) for lv in rep['levels']])))


if __name__ == '__main__':
    main()
