"""Timing of the mesh simplification (points2surf_amd/simplify.py: p2s_mesh_simplify) on one device.  The mesh is the engine's
own 256^3 iso-surface of a stand-in cloud (synth.standin_cloud of the fixture cloud, synthetic p2s_max weights), about 1 M
faces, reduced to ``--max_faces`` (100,000).  Timed with the mesh on the device: the whole call (the search over R and the
final pass) and the final pass alone (the R found, given); the call synchronises its stream, and every run is bracketed by a
device synchronise: two warm-up runs, then ``--reps`` runs; median, minimum and maximum.  The two-sided Hausdorff distance of
the result to the input comes from ``metrics.mesh_distances`` (sampled surfaces), in units of the cell size h.  The numpy
model's time on the 20,480-face torus of the tests is printed as CONTEXT ONLY: it is a test oracle, not a predecessor.
One JSON line.
    python tools/simplify_bench.py [--max_faces N] [--reps N] [--res 256] [--placement quadric|mean]"""
import argparse
import json
import os
import sys
import tempfile
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
    ap.add_argument('--max_faces', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--placement', choices=('quadric', 'mean'), default='quadric')
    ap.add_argument('--samples', type=int, default=10000)
    args = ap.parse_args()
    assert args.reps >= 5
    import torch
    import simplify_model
    from points2surf_amd import engine, metrics, ply, simplify, synth
    base = np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy'))
    cloud = engine.Cloud(synth.standin_cloud(base, 0))
    w, cfg = synth.make_weights('p2s_max')
    sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), args.res, 3)
    vol, _ = engine.sdf_volume(q, sdf, args.res, 5, 13.0, clamp=True)
    v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
    v, f = v.contiguous(), f.contiguous()
    torch.cuda.synchronize()
    kw = dict(max_faces=args.max_faces, placement=args.placement)
    vo, fo, rep = simplify.simplify(v, f, **kw)
    R = rep['resolution']
    row = dict(mesh='standin_000 at %d^3' % args.res, placement=args.placement, max_faces=args.max_faces, report=rep)
    row['whole_call'] = timed(lambda: simplify.simplify(v, f, **kw), args.reps)
    row['final_pass_alone'] = timed(lambda: simplify.simplify(v, f, resolution=R, placement=args.placement), args.reps)
    vn = v.cpu().numpy()
    ext = float((vn.max(0).astype(np.float64) - vn.min(0).astype(np.float64)).max())
    h = ext / max(R, 1)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, 'out.ply'), os.path.join(tmp, 'in.ply')
        ply.write_ply(a, vo.cpu().numpy(), fo.cpu().numpy())
        ply.write_ply(b, vn, f.cpu().numpy())
        h_or, h_ro, hd, _ = metrics.mesh_distances(a, b, samples_per_model=args.samples, seed=0)
    row.update(cell_size=h, hausdorff_out_to_in_h=h_or / h, hausdorff_in_to_out_h=h_ro / h, hausdorff_h=hd / h,
               hausdorff_samples=args.samples)
    tv, tf = simplify_model.torus()
    t = time.perf_counter()
    simplify_model.simplify(tv, tf, max_faces=2000)
    row['context_only_numpy_model_20k_faces_ms'] = (time.perf_counter() - t) * 1e3
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
