"""Timing and effect of p2s_mesh_smooth on one device.  First measurements: no earlier number exists to compare
with, nothing is gated.

  recon   the engine's own 256^3 iso-surface of a stand-in cloud (the mesh of tools/holes_bench.py) after
          ``clean.repair(max_hole_edges=0)`` (weld, orient, no fill) and ``manifold.manifold`` (split).  ``smooth.smooth`` at 0
          iterations (the setup alone: validation, edge table, classes, and no rows), at 10 and at 50 iterations in mode
          'fixed' -- the cost of a half-step is the difference of the two over 80 half-steps --, at 10 iterations in 'curve' and
          in 'free'; ``components.components`` beside them in the same run.  Area and signed volume before and after the
          defaults, the largest displacement in voxels (2 / res).
  sphere  a unit icosphere of 163,842 vertices with Gaussian noise of 0.3 mean edge lengths on every coordinate: the radial
          RMS (|p| - 1) and the mean angle between a face normal and the direction of its centroid, before and after 10
          Taubin iterations and after 20 Laplacian half-steps (lambda 0.5), with the change of the volume.
  cone    long rows: a ring of 3,000 and one of ``--ring`` vertices, each closed by two apexes that have the whole ring as
          neighbours; 10 and 50 iterations, per half-step as above.

Every call ends in a device synchronise: two warm-up runs, then ``--reps`` runs; median, minimum and maximum.  One JSON line.
The share of p2s_smooth_step_kernel comes from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/smooth_bench.py --only recon --reps 1
    python tools/smooth_bench.py [--only recon|sphere|cone] [--reps N] [--res 256] [--ring 100000]"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
FIX = os.path.join(REPO, 'tests', 'golden', 'abc_minimal')


def per_half_step(t10, t50, per_iteration=2):
    return (t50['median_ms'] - t10['median_ms']) / (40 * per_iteration)


def sphere_errors(v, f):
    """radial RMS against the unit sphere; the mean angle (degrees) between a face normal and its centroid's direction"""
    v = np.asarray(v, np.float64)
    p = v[np.asarray(f, np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    c = p.mean(axis=1)
    cos = np.einsum('ij,ij->i', n, c) / (np.linalg.norm(n, axis=1) * np.linalg.norm(c, axis=1))
    return dict(radial_rms=float(np.sqrt(np.mean((np.linalg.norm(v, axis=1) - 1.0) ** 2))),
                normal_angle_deg=float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=('recon', 'sphere', 'cone'), default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--ring', type=int, default=100000)
    args = ap.parse_args()
    import torch
    import smooth_model as SM
    from components_bench import timed
    from points2surf_amd import clean, components, engine, manifold, smooth, synth
    row = {}
    if args.only in (None, 'recon'):
        base = np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy'))
        cloud = engine.Cloud(synth.standin_cloud(base, 0))
        w, cfg = synth.make_weights('p2s_max')
        sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), args.res, 3)
        vol, _ = engine.sdf_volume(q, sdf, args.res, 5, 13.0, clamp=True)
        v0, f0, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
        v1, f1, _, _ = clean.repair(v0.contiguous(), f0.contiguous(), max_hole_edges=0)
        v, f, _ = manifold.manifold(v1, f1, edges='split')
        v, f = v.contiguous(), f.contiguous()
        torch.cuda.synchronize()
        vo, _, rep = smooth.smooth(v, f)
        before, after = components.components(v, f)[1], components.components(vo, f)[1]
        r = dict(mesh='standin_000 at %d^3, repaired without fill, split' % args.res, verts=int(v.shape[0]), faces=int(f.shape[0]),
                 report=rep, max_displacement_voxels=rep['max_displacement'] / (2.0 / args.res),
                 area_in=float(before['area'].sum()), area_out=float(after['area'].sum()),
                 volume_in=float(before['volume'].sum()), volume_out=float(after['volume'].sum()))
        r['setup_0_iterations'] = timed(lambda: smooth.smooth(v, f, iterations=0), args.reps)
        r['fixed_10'] = timed(lambda: smooth.smooth(v, f, iterations=10), args.reps)
        r['fixed_50'] = timed(lambda: smooth.smooth(v, f, iterations=50), args.reps)
        r['half_step_ms'] = per_half_step(r['fixed_10'], r['fixed_50'])
        r['curve_10'] = timed(lambda: smooth.smooth(v, f, iterations=10, boundary='curve'), args.reps)
        r['free_10'] = timed(lambda: smooth.smooth(v, f, iterations=10, boundary='free'), args.reps)
        r['components'] = timed(lambda: components.components(v, f), args.reps)
        row['recon'] = r
    if args.only in (None, 'sphere'):
        sv, sf = SM.icosphere(7)
        a, b, _ = SM.edges(sf)
        edge = float(np.linalg.norm(sv[a].astype(np.float64) - sv[b].astype(np.float64), axis=1).mean())
        noisy = (sv.astype(np.float64) + np.random.default_rng(7).normal(0.0, 0.3 * edge, sv.shape)).astype(np.float32)
        tv, tf = torch.from_numpy(noisy).cuda(), torch.from_numpy(sf).cuda()
        r = dict(mesh='icosphere, 7 subdivisions', verts=int(len(sv)), faces=int(len(sf)), mean_edge=edge, sigma=0.3 * edge,
                 clean=sphere_errors(sv, sf), noisy=sphere_errors(noisy, sf))
        vol = SM.signed_volume(noisy, sf)
        for name, kw in (('taubin_10', dict(iterations=10)), ('laplacian_20', dict(iterations=20, mu=0.0))):
            vo, _, rep = smooth.smooth(tv, tf, **kw)
            vo = vo.cpu().numpy()
            r[name] = dict(sphere_errors(vo, sf), half_steps=rep['half_steps'], max_displacement=rep['max_displacement'],
                           volume_change=SM.signed_volume(vo, sf) / vol - 1.0, **timed(lambda: smooth.smooth(tv, tf, **kw), args.reps))
        row['sphere'] = r
    if args.only in (None, 'cone'):
        r = {}
        for n in (3000, args.ring):
            cv, cf = SM.cone(n)
            tv, tf = torch.from_numpy(cv).cuda(), torch.from_numpy(cf).cuda()
            t10 = timed(lambda: smooth.smooth(tv, tf, iterations=10), args.reps)
            t50 = timed(lambda: smooth.smooth(tv, tf, iterations=50), args.reps)
            r['ring_%d' % n] = dict(verts=n + 2, max_neighbours=smooth.smooth(tv, tf, iterations=1)[2]['max_neighbours'], it_10=t10, it_50=t50,
                                    half_step_ms=per_half_step(t10, t50))
        row['cone'] = r
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
