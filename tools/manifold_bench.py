"""Timing of p2s_mesh_manifold on one device.  First measurements: no earlier number exists to compare with,
nothing is gated.

  ``manifold.manifold`` in mode 2 (``edges='split'``) and mode 3 (``edges='remove'``) on the engine's own 256^3 iso-surface of a
  stand-in cloud (the mesh of tools/simplify_bench.py and tools/components_bench.py) and on its simplification to at most
  ``--max_faces`` (100,000) faces, which holds the edges of more than two faces that clustering creates.  Beside them
  ``components.components`` on the same meshes: a yardstick of the same class (edge table + union-find + sort).  The report of
  every call is printed with its hook rounds.

Every call ends in a device synchronise: two warm-up runs, then ``--reps`` runs; median, minimum and maximum.  One JSON line.
    python tools/manifold_bench.py [--reps N] [--res 256] [--max_faces 100000]"""
import argparse
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
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--max_faces', type=int, default=100000)
    args = ap.parse_args()
    import torch
    from components_bench import timed
    from points2surf_amd import components, engine, manifold, simplify, synth
    base = np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy'))
    cloud = engine.Cloud(synth.standin_cloud(base, 0))
    w, cfg = synth.make_weights('p2s_max')
    sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), args.res, 3)
    vol, _ = engine.sdf_volume(q, sdf, args.res, 5, 13.0, clamp=True)
    v, f, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
    v, f = v.contiguous(), f.contiguous()
    sv, sf, srep = simplify.simplify(v, f, max_faces=args.max_faces)
    sv, sf = sv.contiguous(), sf.contiguous()
    torch.cuda.synchronize()
    row = {}
    for name, (mv, mf) in (('standin_000 at %d^3' % args.res, (v, f)), ('simplified to <= %d faces' % args.max_faces, (sv, sf))):
        r = dict(verts=int(mv.shape[0]), faces=int(mf.shape[0]))
        for key, kw in (('mode2_split', dict(edges='split')), ('mode3_remove_split', dict(edges='remove'))):
            r[key] = dict(report=manifold.manifold(mv, mf, **kw)[2], **timed(lambda: manifold.manifold(mv, mf, **kw), args.reps))
        r['components'] = dict(hook_rounds=components.components(mv, mf)[2]['hook_rounds'],
                               **timed(lambda: components.components(mv, mf), args.reps))
        row[name] = r
    row['simplify_report'] = {k: srep[k] for k in ('resolution', 'nonmanifold_edges_out', 'boundary_edges_out')}
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
