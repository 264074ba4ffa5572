"""Timing of the GT-distance path (points2surf_amd/gt_sdf.py): handle build, 2,000 queries and the full 256^3 query grid of
the test shape against each fixture mesh and against the engine's own 256^3 mesh, indexed next to exhaustive.  HIP events,
one warm-up, median of three; one JSON line per case.  Then the winding number of the same query sets on the same handles: the
tree walk (tau = 2^-10 and the largest tau, 0.25) next to the exact sum, with the nodes accepted and triangles evaluated per
query and the share of queries re-decided exactly.
    python tools/gt_sdf_bench.py [--skip-large] [--no-exhaustive-large] [--winding-only]"""
import argparse
import glob
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FIX = os.path.join(REPO, 'tests', 'golden', 'abc_minimal')


def timed(fn, reps=3, warm=True):
    import torch
    if warm:
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-large', action='store_true')
    ap.add_argument('--no-exhaustive-large', action='store_true', help='skip grid x 0.92 M faces exhaustively (~3e11 tests)')
    ap.add_argument('--winding-only', action='store_true', help='skip the distance rows')
    args = ap.parse_args()
    import torch
    from points2surf_amd import engine, gt_sdf, ply, synth
    pts = np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy'))
    cloud = engine.Cloud(pts)
    grid = cloud.query_grid(256, 3).contiguous()
    few = torch.from_numpy(np.load(glob.glob(os.path.join(FIX, '05_query_pts', '00994122*'))[0]).astype(np.float32)).cuda()
    meshes = [(os.path.basename(f)[:8],) + tuple(ply.read_ply(f)) for f in sorted(glob.glob(os.path.join(FIX, '03_meshes', '*.ply')))]
    if not args.skip_large:
        w, cfg = synth.make_weights('p2s_max')
        sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), 256, 3)
        vol, _ = engine.sdf_volume(q, sdf, 256, 5, 13.0, clamp=True)
        v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
        meshes.append(('engine256',) + ply.merge_vertices(v.cpu().numpy(), f.cpu().numpy()))
    for name, v, f in meshes:
        vt = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        ft = torch.from_numpy(np.ascontiguousarray(f).astype(np.int32)).cuda()
        build_ms = timed(lambda: gt_sdf.TriMesh(vt, ft).close())
        mesh = gt_sdf.TriMesh(vt, ft)
        info = mesh.info()
        for label, q in (('2000', few), ('grid256', grid)):
            for signed in () if args.winding_only else (False, True) if info['closed'] else (False,):
                row = dict(mesh=name, faces=info['n_faces'], grid=info['grid'], components=info['components'], build_ms=build_ms,
                           queries=int(q.shape[0]), set=label, signed=signed)
                row['index_ms'] = timed(lambda: mesh.distance(q, signed=signed, method='index'))
                row['tests_per_query'] = mesh.info()['tests'] / q.shape[0]
                row['n_winding'] = mesh.n_winding
                if not (name == 'engine256' and label == 'grid256' and args.no_exhaustive_large):
                    row['exhaustive_ms'] = timed(lambda: mesh.distance(q, signed=signed, method='exhaustive'),
                                                 reps=1 if name == 'engine256' and label == 'grid256' else 3)
                print(json.dumps(row), flush=True)
        for label, q in (('2000', few), ('grid256', grid)):
            big = name == 'engine256' and label == 'grid256'          # ~3e11 atan2 per call: one timed call, no warm-up
            row = dict(kind='winding', mesh=name, faces=info['n_faces'], grid=info['grid'], queries=int(q.shape[0]), set=label)
            for tau in (2.0 ** -10, 0.25):
                key = 'tree_tau%g' % tau
                row[key + '_ms'] = timed(lambda: mesh.winding(q, method='tree', tau=tau), reps=1 if big else 3, warm=not big)
                st = mesh.winding(q, method='tree', tau=tau, want_stats=True)[1] if not big else None
                if st is not None:
                    row[key + '_nodes_per_query'] = st['accepted'] / q.shape[0]
                    row[key + '_triangles_per_query'] = st['triangles'] / q.shape[0]
                    row[key + '_redecided_share'] = st['redecided'] / q.shape[0]
            if not (big and args.no_exhaustive_large):
                row['exhaustive_ms'] = timed(lambda: mesh.winding(q, method='exhaustive'), reps=1 if big else 3, warm=not big)
            print(json.dumps(row), flush=True)
        mesh.close()


if __name__ == '__main__':
    main()
