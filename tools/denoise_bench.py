"""Timing and effect of p2s_mesh_denoise on one device, with p2s_mesh_smooth beside it in the same run.  First
measurements: no earlier number exists to compare with, nothing is gated.

  recon   the engine's own 256^3 iso-surface of a stand-in cloud (the mesh of tools/smooth_bench.py) after
          ``clean.repair(max_hole_edges=0)`` (weld, orient, no fill) and ``manifold.manifold`` (split).  ``denoise.denoise`` at
          its defaults (T 0.5, 10 + 10 iterations), at 0 + 0 iterations (the setup alone: validation, edge table, normals,
          the sort of the rows, classes), at 50 + 10 and at 10 + 50: a normal iteration and a vertex iteration cost the
          difference to the defaults over 40.  10 Taubin iterations of ``smooth.smooth`` beside them.  The bytes that one launch
          of either hot kernel asks for, from the mesh's own counts.  Area and signed volume before and after the defaults, the
          largest displacement in voxels (2 / res).
  cube    the unit cube of ``--quads`` x ``--quads`` quads per side, each split ``--split`` times (one quad -> four), with
          Gaussian noise of 0.2 edge lengths on every coordinate: the mean angle between the face normals and those of the
          clean cube, before, after the defaults, and after 10 Taubin iterations; the times of both.

Every call ends in a device synchronise: two warm-up runs, then ``--reps`` runs; median, minimum and maximum.  One JSON line.
The shares of the two hot kernels come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/denoise_bench.py --only recon --reps 1
    python tools/denoise_bench.py [--only recon|cube] [--reps N] [--res 256] [--quads 12] [--split 3]"""
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


def launch_bytes(V, f):
    """what one launch of either hot kernel asks the memory system for, from the counts of the mesh: dict of byte counts"""
    import denoise_model as DM
    f = np.asarray(f, np.int64)
    F = len(f)
    deg = np.bincount(f.reshape(-1), minlength=V)
    row_entries = int((deg[f.reshape(-1)]).sum())                       # the column indices that the merges of all faces read
    fstart, _ = DM.neighbours(V, f)
    visits = int(fstart[-1])                                            # the neighbour normals gathered: sum of |N(i)|
    filt = dict(faces=12 * F, row_starts=24 * F, columns=4 * row_entries, own_normals=12 * F, neighbour_normals=12 * visits, written=12 * F)
    vert = dict(classes=V, row_starts=8 * V, own_positions=12 * V, columns=4 * 3 * F, normals=12 * 3 * F, corners=12 * 3 * F,
                corner_positions=36 * 3 * F, written=12 * V)
    return dict(neighbour_visits=visits, mean_neighbours=visits / max(F, 1), filter=filt, filter_total=sum(filt.values()),
                filter_compulsory=12 * F + 4 * 3 * F + 8 * V + 12 * F + 12 * F, vertex=vert, vertex_total=sum(vert.values()),
                vertex_compulsory=V + 8 * V + 12 * V + 4 * 3 * F + 12 * F + 12 * F + 12 * V)


def both_timed(timed, denoise, smooth, v, f, reps):
    t = dict(default=timed(lambda: denoise.denoise(v, f), reps),
             setup_0_0=timed(lambda: denoise.denoise(v, f, normal_iterations=0, vertex_iterations=0), reps),
             normal_50=timed(lambda: denoise.denoise(v, f, normal_iterations=50), reps),
             vertex_50=timed(lambda: denoise.denoise(v, f, vertex_iterations=50), reps),
             taubin_10=timed(lambda: smooth.smooth(v, f), reps))
    t['normal_iteration_ms'] = (t['normal_50']['median_ms'] - t['default']['median_ms']) / 40
    t['vertex_iteration_ms'] = (t['vertex_50']['median_ms'] - t['default']['median_ms']) / 40
    t['setup_share'] = t['setup_0_0']['median_ms'] / t['default']['median_ms']
    return t


def subdivided(v, f, times):
    """every triangle into four by its edge midpoints, ``times`` times; shared edges share their midpoint"""
    v = [tuple(p) for p in np.asarray(v, np.float64)]
    f = np.asarray(f, np.int64).tolist()
    for _ in range(times):
        mid, g = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                v.append(tuple((np.array(v[i]) + np.array(v[j])) / 2.0))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = g
    return np.array(v, np.float64), np.array(f, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=('recon', 'cube'), default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--quads', type=int, default=12)
    ap.add_argument('--split', type=int, default=3)
    args = ap.parse_args()
    import torch
    import denoise_model as DM
    from components_bench import timed
    from points2surf_amd import clean, components, denoise, engine, manifold, smooth, synth
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
        vo, _, rep = denoise.denoise(v, f)
        before, after = components.components(v, f)[1], components.components(vo, f)[1]
        r = dict(mesh='standin_000 at %d^3, repaired without fill, split' % args.res, verts=int(v.shape[0]), faces=int(f.shape[0]),
                 report=rep, max_displacement_voxels=rep['max_displacement'] / (2.0 / args.res),
                 area_in=float(before['area'].sum()), area_out=float(after['area'].sum()),
                 volume_in=float(before['volume'].sum()), volume_out=float(after['volume'].sum()))
        so = smooth.smooth(v, f)[0]
        s_after = components.components(so, f)[1]
        r['taubin_area_out'], r['taubin_volume_out'] = float(s_after['area'].sum()), float(s_after['volume'].sum())
        r.update(both_timed(timed, denoise, smooth, v, f, args.reps))
        r['bytes_per_launch'] = launch_bytes(int(v.shape[0]), f.cpu().numpy())
        row['recon'] = r
    if args.only in (None, 'cube'):
        cv, cf = DM.cube(args.quads)
        cv, cf = subdivided(cv, cf, args.split)
        edge = 1.0 / (args.quads * 2 ** args.split)
        noisy = (cv + np.random.RandomState(3).normal(0.0, 0.2 * edge, cv.shape)).astype(np.float32)
        tv, tf = torch.from_numpy(noisy).cuda(), torch.from_numpy(cf).cuda()
        vo, _, rep = denoise.denoise(tv, tf)
        so = smooth.smooth(tv, tf)[0]
        r = dict(mesh='cube, %d x %d quads per side, split %d times' % (args.quads, args.quads, args.split), verts=int(len(cv)),
                 faces=int(len(cf)), sigma=0.2 * edge, report=rep,
                 normal_error_deg=dict(noisy=DM.normal_error_deg(noisy, cf, cv), denoised=DM.normal_error_deg(vo.cpu().numpy(), cf, cv),
                                       taubin_10=DM.normal_error_deg(so.cpu().numpy(), cf, cv)))
        r.update(both_timed(timed, denoise, smooth, tv, tf, args.reps))
        row['cube'] = r
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
