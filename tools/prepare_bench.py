"""Timing of the raw-scan stages (points2surf_amd.prepare: p2s_prepare_*) on one device.  The cloud is the stand-in blob
(``synth.make_cloud``) of ``--points`` (1,000,000) points, 0.5 % of them replaced by uniform outliers in a box 3 times the
object's size and five by returns at 100 times its extent.

  crop on    every stage on the full cloud: non-finite, crop, outliers (k = 16), random and voxel thinning to 150,000,
             unit cube, and ``prepare`` as a whole -- one warm-up, then ``--reps`` calls each, on the host clock around a call
             that ends in a device synchronise; medians.
  crop off   the five far returns stay, the neighbour index (at most 128^3 cells over the bounding box) puts the whole object
             into a handful of cells and every query scans nearly every point: the outlier stage is near-quadratic there, so it
             is timed on the first ``--quadratic_points`` (150,000) points only, once.

Beside them scipy's ``cKDTree.query(k + 1, workers=16)`` on this machine's CPU for the same statistic on the cropped cloud, and
whether the keep flags equal the ones derived from it: scipy's distances may differ in the last ulp, so the differing points
are counted, not asserted on.  No ratio is gated.  One JSON line.
    python tools/prepare_bench.py [--points N] [--reps N] [--quadratic_points N] [--no_cpu]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def standin_scan(n, seed=0):
    from points2surf_amd import synth
    rng = np.random.default_rng(seed + 1)
    p = synth.make_cloud(n, seed=seed).astype(np.float32)
    m = int(round(0.005 * n))
    who = rng.permutation(n)
    p[who[:m]] = rng.uniform(-1.5, 1.5, (m, 3)).astype(np.float32)
    p[who[m:m + 5]] = (100.0 * rng.choice([-1.0, 1.0], (5, 3)) * rng.uniform(0.5, 1.0, (5, 3))).astype(np.float32)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--quadratic_points', type=int, default=150000)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    import torch
    from points2surf_amd import prepare
    k = args.k
    scan = standin_scan(args.points)
    raw = torch.from_numpy(scan).cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def median(fn, reps=args.reps):
        fn()
        ms = [timed(fn)[0] for _ in range(reps)]
        return dict(ms=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))

    cropped = prepare.crop(raw, 0.01, 1.0)[0]
    clean, _, info = prepare.remove_outliers(cropped, k, 2.0, want_report=True)
    res = dict(points=int(raw.shape[0]), k=k, reps=args.reps, cropped=int(raw.shape[0] - cropped.shape[0]),
               outliers=int(cropped.shape[0] - clean.shape[0]), mean=info['mean'], std=info['std'], threshold=info['threshold'])
    res['stages_ms'] = dict(
        finite=median(lambda: prepare.drop_nonfinite(raw)),
        crop=median(lambda: prepare.crop(raw, 0.01, 1.0)),
        outliers=median(lambda: prepare.remove_outliers(cropped, k, 2.0)),
        thin_random=median(lambda: prepare.random_thin(clean, 150000, 42)),
        thin_voxel=median(lambda: prepare.voxel_thin(clean, 150000)),
        normalize=median(lambda: prepare.normalize(clean)),
        prepare_random=median(lambda: prepare.prepare(raw, k=k)),
        prepare_voxel=median(lambda: prepare.prepare(raw, k=k, thin='voxel')))
    res['voxel_R'] = prepare.voxel_thin(clean, 150000, want_report=True)[2]['R']
    # crop off: near-quadratic (see above), a smaller cloud, one call
    far = scan[(np.abs(scan) > 10.0).any(axis=1)]
    small = torch.from_numpy(np.concatenate([scan[(np.abs(scan) <= 10.0).all(axis=1)][:args.quadratic_points - len(far)], far])).cuda()
    small_cropped = prepare.crop(small, 0.01, 1.0)[0]
    res['crop_off'] = dict(points=int(small.shape[0]), outliers_ms=timed(lambda: prepare.remove_outliers(small, k, 2.0))[0],
                           outliers_after_crop_ms=median(lambda: prepare.remove_outliers(small_cropped, k, 2.0))['ms'])
    if not args.no_cpu:
        from scipy.spatial import cKDTree
        x = cropped.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        dist = cKDTree(x).query(x, k + 1, workers=16)[0]
        res['scipy_query_ms'] = 1e3 * (time.perf_counter() - t0)
        d = dist.sum(axis=1) / k
        keep = d <= d.mean() + 2.0 * d.std()
        mine = np.zeros(len(x), bool)
        mine[prepare.remove_outliers(cropped, k, 2.0)[1].cpu().numpy()] = True
        res['flags_differ_from_scipy'] = int((keep != mine).sum())
        res['flags_equal_scipy'] = bool((keep == mine).all())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
