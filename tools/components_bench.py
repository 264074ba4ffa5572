"""Timing of the component calls on one device.  First measurements: no earlier number exists to compare with,
nothing is gated.

  mesh      ``components.components`` and ``components.filter_mesh`` (defaults of the command line: min_area_share 0.01) on the
            engine's own 256^3 iso-surface of a stand-in cloud (the mesh of tools/simplify_bench.py), on the device.
  clusters  ``prepare.remove_small_clusters`` on the stand-in blob of ``--points`` (1,000,000) points with 0.5 % of them moved
            into 25 clumps, after the crop and the outlier stage of ``prepare``, at the automatic radius (3 times that stage's
            mean) and min_points 1000.  Beside the time: the points in the 27 cells around a point, averaged over the points
            (counted on the host in numpy, over cells of the radius) -- the pair kernel's first round tests half of them.

Every call ends in a device synchronise: two warm-up runs, then ``--reps`` runs; median, minimum and maximum.  One JSON line.
The per-kernel shares come from a run of its own under the profiler, one workload at a time:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/components_bench.py --only clusters --reps 1
    python tools/components_bench.py [--only mesh|clusters] [--points N] [--reps N] [--res 256]"""
import argparse
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


def clumped_scan(n, seed=0, clumps=25):
    from points2surf_amd import synth
    rng = np.random.default_rng(seed + 1)
    p = synth.make_cloud(n, seed=seed).astype(np.float32)
    m = int(round(0.005 * n))
    who = rng.permutation(n)[:m]
    centres = rng.uniform(-1.5, 1.5, (clumps, 3))
    p[who] = (centres[rng.integers(0, clumps, m)] + rng.normal(0.0, 0.01, (m, 3))).astype(np.float32)
    return p


def candidates_per_point(points, radius):
    p = points.astype(np.float64)
    cell = np.floor((p - p.min(0)) / radius).astype(np.int64) + 1
    dims = cell.max(0) + 2
    key = (cell[:, 0] * dims[1] + cell[:, 1]) * dims[2] + cell[:, 2]
    uniq, count = np.unique(key, return_counts=True)
    total = 0
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                want = uniq + (dx * dims[1] + dy) * dims[2] + dz
                at = np.minimum(np.searchsorted(uniq, want), uniq.size - 1)
                total += int((count * np.where(uniq[at] == want, count[at], 0)).sum())
    return total / p.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=('mesh', 'clusters'), default=None)
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=256)
    args = ap.parse_args()
    import torch
    from points2surf_amd import components, engine, prepare, synth
    row = {}
    if args.only in (None, 'mesh'):
        base = np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy'))
        cloud = engine.Cloud(synth.standin_cloud(base, 0))
        w, cfg = synth.make_weights('p2s_max')
        sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), args.res, 3)
        vol, _ = engine.sdf_volume(q, sdf, args.res, 5, 13.0, clamp=True)
        v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
        v, f = v.contiguous(), f.contiguous()
        torch.cuda.synchronize()
        _, st, rep = components.components(v, f)
        _, _, frep = components.filter_mesh(v, f, min_area_share=0.01)
        row['mesh'] = dict(mesh='standin_000 at %d^3' % args.res, verts=int(v.shape[0]), faces=int(f.shape[0]), report=rep,
                           components_kept=frep['components_kept'], faces_out=frep['faces_out'], cavities=frep['cavities'],
                           largest_removed_area_share=frep['largest_removed_area_share'],
                           components=timed(lambda: components.components(v, f), args.reps),
                           filter_mesh=timed(lambda: components.filter_mesh(v, f, min_area_share=0.01), args.reps))
    if args.only in (None, 'clusters'):
        raw = torch.from_numpy(clumped_scan(args.points)).cuda()
        cropped = prepare.crop(raw, 0.01, 1.0)[0]
        clean, _, info = prepare.remove_outliers(cropped, 16, 2.0, want_report=True)
        radius = 3.0 * info['mean']
        out, _, rep = prepare.remove_small_clusters(clean, radius, 1000, want_report=True)
        rep.pop('labels')
        row['clusters'] = dict(points=int(clean.shape[0]), radius=radius, mean_neighbour_distance=info['mean'], report=rep,
                               points_out=int(out.shape[0]), candidates_per_point=candidates_per_point(clean.cpu().numpy(), radius),
                               remove_small_clusters=timed(lambda: prepare.remove_small_clusters(clean, radius, 1000), args.reps))
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
