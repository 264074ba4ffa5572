"""Timing of p2s_mesh_fill_holes on one device.  First measurements: no earlier number exists to compare with,
nothing is gated.

  recon      the engine's own 256^3 iso-surface of a stand-in cloud (the mesh of tools/manifold_bench.py) after
             ``clean.repair(max_hole_edges=0)`` (weld, orient, no fill) and ``manifold.manifold`` (split): its loops by size;
             ``holes.fill`` at 30 and at 128 edges with the holes filled / too long / blocked, whether the result is closed
             and whether ``TriMesh.voxelize`` accepts it; beside them ``clean.repair(max_hole_edges=30)`` (the fan) and
             ``components.components`` on the same mesh in the same run, and ``holes.fill`` at 0 edges: the call without
             candidates, so without the dynamic programme, the emit and the second edge table.
  synthetic  1,000 holes of 128 edges in one mesh: the worst case of the dynamic programme.

Every call ends in a device synchronise: two warm-up runs, then ``--reps`` runs; median, minimum and maximum.  One JSON line.
The share of p2s_hf_dp_kernel comes from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/holes_bench.py --only synthetic --reps 1
    python tools/holes_bench.py [--only recon|synthetic] [--reps N] [--res 256] [--holes 1000]"""
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


def accepted_by_voxelize(v, f, res=128):
    """True, or the words of the refusal; 128 is the IoU grid of the quality report"""
    from points2surf_amd import _lib, gt_sdf
    mesh = gt_sdf.TriMesh(v, f)
    try:
        mesh.voxelize(res)
        return True
    except _lib.P2SError as e:
        return ' '.join(str(e).split())
    finally:
        mesh.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=('recon', 'synthetic'), default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--holes', type=int, default=1000)
    args = ap.parse_args()
    import torch
    from components_bench import timed
    from points2surf_amd import clean, components, engine, holes, manifold, synth
    row = {}
    if args.only in (None, 'recon'):
        base = np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy'))
        cloud = engine.Cloud(synth.standin_cloud(base, 0))
        w, cfg = synth.make_weights('p2s_max')
        sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), args.res, 3)
        vol, _ = engine.sdf_volume(q, sdf, args.res, 5, 13.0, clamp=True)
        v0, f0, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
        v0, f0 = v0.contiguous(), f0.contiguous()
        v1, f1, _, rrep = clean.repair(v0, f0, max_hole_edges=0)
        v, f, mrep = manifold.manifold(v1, f1, edges='split')
        v, f = v.contiguous(), f.contiguous()
        torch.cuda.synchronize()
        r = dict(mesh='standin_000 at %d^3, repaired without fill, split' % args.res, verts=int(v.shape[0]), faces=int(f.shape[0]),
                 boundary_edges=mrep['boundary_edges_out'], repair_holes_left=rrep.get('holes_left'))
        table = holes.fill(v, f, max_hole_edges=0, want_holes=True)[2]
        sizes = table['holes'][:, 1].cpu().numpy()
        r['loops_by_size'] = {str(int(n)): int(c) for n, c in zip(*np.unique(sizes, return_counts=True))}
        r['boundary_groups'] = table['boundary_groups_out']
        for K in (30, 128):
            vo, fo, rep = holes.fill(v, f, max_hole_edges=K)
            closed = rep['boundary_edges_out'] == 0 and rep['nonmanifold_edges'] == 0
            r['fill_%d' % K] = dict(report=rep, closed=closed, voxelize_accepts=accepted_by_voxelize(vo, fo),
                                    **timed(lambda: holes.fill(v, f, max_hole_edges=K), args.reps))
        r['fill_0_no_candidates'] = timed(lambda: holes.fill(v, f, max_hole_edges=0), args.reps)
        fan = clean.repair(v, f, max_hole_edges=30)
        r['repair_fan_30'] = dict(holes_filled=fan[3]['holes_filled'], faces_added=fan[3]['faces_added'], watertight=fan[3]['watertight'],
                                  voxelize_accepts=accepted_by_voxelize(fan[0], fan[1]),
                                  **timed(lambda: clean.repair(v, f, max_hole_edges=30), args.reps))
        r['components'] = timed(lambda: components.components(v, f), args.reps)
        row['recon'] = r
    if args.only in (None, 'synthetic'):
        import holes_model as HM
        rng = np.random.default_rng(128)
        sv, sf = HM.join([HM.cup(HM.random_loop(128, rng) + np.float32(4.0 * i)) for i in range(args.holes)])
        sv, sf = torch.from_numpy(sv).cuda(), torch.from_numpy(sf).cuda()
        rep = holes.fill(sv, sf, max_hole_edges=128)[2]
        row['synthetic'] = dict(mesh='%d holes of 128 edges' % args.holes, verts=int(sv.shape[0]), faces=int(sf.shape[0]), report=rep,
                                fill_128=timed(lambda: holes.fill(sv, sf, max_hole_edges=128), args.reps),
                                fill_0_no_candidates=timed(lambda: holes.fill(sv, sf, max_hole_edges=0), args.reps))
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
