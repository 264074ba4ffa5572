"""Timing of the normals from the cloud alone (points2surf_amd.normals: p2s_normals_estimate, p2s_normals_orient) on one
device, on a fixture cloud (``--stem``; default the largest, 86,648 points) at ``--k`` (16): one warm-up, then ``--reps`` rounds
of three calls, each on the host clock around a call that ends in a device synchronise -- the kNN alone (p2s_knn_patch, ids
only: what both entry points run first), the estimate (kNN + covariance and eigenvectors) and the orientation (kNN + Boruvka
rounds).  Medians; covariance and orientation also less the kNN.  Next to them the gather traffic of the covariance kernel
(per point k ids and k points, 16 bytes a neighbour) and its time at 6.3 TB/s, the Boruvka rounds, the components and,
where the shape has a mesh, the error against the normals of the nearest faces.  The kernels' own times come from a
``rocprofv3 --kernel-trace --stats`` run of this tool.  One JSON line.
    python tools/normals_bench.py [--k K] [--reps N] [--stem NAME]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FIX = os.path.join(REPO, 'tests', 'golden', 'abc_minimal')
HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--stem', default=None, help='shape of tests/golden/abc_minimal (default: the one with the largest cloud)')
    args = ap.parse_args()
    import torch
    from points2surf_amd import baseline, engine, normals, ply
    stems = sorted(f[:-len('.xyz.npy')] for f in os.listdir(os.path.join(FIX, '04_pts')) if f.endswith('.xyz.npy'))
    stem = args.stem or max(stems, key=lambda t: os.path.getsize(os.path.join(FIX, '04_pts', t + '.xyz.npy')))
    pts = np.load(os.path.join(FIX, '04_pts', stem + '.xyz.npy')).astype(np.float32)
    n, k = int(pts.shape[0]), args.k
    cloud = engine.Cloud(pts)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    calls = dict(knn=lambda: cloud.knn_patch(cloud.pts, k, want_patch=False),
                 estimate=lambda: normals.estimate(cloud, k=k, orient='none'),
                 orient=lambda: normals.orient(cloud, nrm, k=k, want_report=True))
    nrm = normals.estimate(cloud, k=k, orient='none')[0]
    ms = {name: [] for name in calls}
    for rep in range(args.reps + 1):
        for name, fn in calls.items():
            t, out = timed(fn)
            if rep:
                ms[name].append(t)
    oriented, report = out
    med = {name: float(np.median(v)) for name, v in ms.items()}
    gather = n * k * 16
    res = dict(shape=stem, points=n, k=k, reps=args.reps, knn_ms=med['knn'], estimate_ms=med['estimate'], orient_ms=med['orient'],
               covariance_ms=med['estimate'] - med['knn'], orientation_ms=med['orient'] - med['knn'],
               spread_ms={name: [float(min(v)), float(max(v))] for name, v in ms.items()},
               gather_bytes=gather, gather_ms_at_6_3_TBps=1e3 * gather / HBM_BYTES_PER_S,
               rounds=report['rounds'], components=report['components'], edges=report['edges'], flipped=report['flipped'])
    f_mesh = os.path.join(FIX, '03_meshes', stem + '.ply')
    if os.path.isfile(f_mesh):
        v, f = ply.read_ply(f_mesh)
        angle, against = baseline.normals_error(oriented.cpu().numpy(), baseline.point_normals(v, f, pts))
        res.update(mean_angle_error_deg=angle, share_against_gt=against)
    cloud.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
