"""Timing of p2s_mesh_render on one device, with p2s_mesh_raycast over the same primary rays beside it in the
same run.  First measurements: no earlier number exists to compare with, nothing is gated.

  mesh     the engine's own 256^3 iso-surface of a stand-in cloud (the mesh of tools/denoise_bench.py), repaired without fill
           and split, as a ``scan.TriMesh``; the camera is ``figure.fit_camera`` at its defaults
  render   1024 x 768 at 2 x 2 samples, flat and smooth, with 0 and with 16 occlusion rays: the raw call on preallocated
           outputs, ms per image, rays per second (primary + occlusion), ray-triangle tests per ray from the call's counters
  raycast  the same primary rays, made on the host by the numpy model's ``sample_rays`` and uploaded once, through
           ``TriMesh.raycast``: the yardstick of the primary pass (which launches the same kernel over a tiled thread order)
  split    occlusion = (16 rays) - (0 rays); the launches of a picture without occlusion are rays + primary + shade + resolve

Every call ends in a device synchronise: two warm-up runs, then ``--reps`` runs; median, minimum and maximum.  One JSON line.
The per-kernel shares come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/figure_bench.py --only flat_k16 --reps 1
    python tools/figure_bench.py [--only flat_k0|flat_k16|smooth_k0|smooth_k16|raycast] [--reps N] [--res 256] [--width W --height H]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
FIX = os.path.join(REPO, 'tests', 'golden', 'abc_minimal')
CONFIGS = {'flat_k0': ('flat', 0), 'flat_k16': ('flat', 16), 'smooth_k0': ('smooth', 0), 'smooth_k16': ('smooth', 16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=tuple(CONFIGS) + ('raycast',), default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--samples', type=int, default=2)
    args = ap.parse_args()
    import torch
    import figure_model as FM
    from components_bench import timed
    from points2surf_amd import _lib, clean, engine, figure, manifold, scan, synth
    base = np.load(os.path.join(FIX, '04_pts', '00994122_57d9d4755722f9d2d7436f0a_trimesh_000.xyz.npy'))
    cloud = engine.Cloud(synth.standin_cloud(base, 0))
    w, cfg = synth.make_weights('p2s_max')
    sdf, q = engine.infer_shape(engine.Model(w, cfg), cloud, engine.Rng(40938661), args.res, 3)
    vol, _ = engine.sdf_volume(q, sdf, args.res, 5, 13.0, clamp=True)
    v0, f0, _ = engine.marching_cubes(vol, model_space=True, fix_inversion=True)
    v1, f1, _, _ = clean.repair(v0.contiguous(), f0.contiguous(), max_hole_edges=0)
    v, f, _ = manifold.manifold(v1, f1, edges='split')
    mesh = scan.TriMesh(v.contiguous(), f.contiguous())
    dev = mesh.device
    W, H, ss = args.width, args.height, args.samples
    n = W * H * ss * ss
    lo, hi = figure.mesh_bounds(mesh)
    cam = figure.fit_camera((lo, hi), aspect=float(W) / float(H))
    row = dict(mesh='standin_000 at %d^3, repaired without fill, split' % args.res, verts=int(v.shape[0]), faces=int(f.shape[0]),
               grid=mesh.info()['grid'], width=W, height=H, samples=ss, primary_rays=n, ao_radius=0.1 * cam['radius'],
               ao_bias=cam['radius'] / 1024.0)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    for name, (shading, K) in CONFIGS.items():
        if args.only not in (None, name):
            continue
        prm = figure.render_params(cam, W, H, ss, K, shading, row['ao_radius'], row['ao_bias'], 0.6, 0.4, (0.8, 0.8, 0.8), (1.0, 1.0, 1.0))
        table = torch.from_numpy(figure.ao_directions(K)).to(dev) if K else None
        st = (ctypes.c_int64 * 8)()

        def call():
            _lib.check(lib.p2s_mesh_render(mesh.handle, ctypes.byref(prm), None, engine._ptr(table), engine._ptr(rgb), None, None, st,
                                           engine._stream_ptr(dev)))
        r = timed(call, args.reps)
        stats = dict(zip(figure.STATS_KEYS, (int(x) for x in st)))
        rays = stats['primary_rays'] + stats['ao_rays']
        r.update(stats, rays=rays, rays_per_second=rays / (r['median_ms'] * 1e-3), tests_per_ray=stats['tests'] / rays,
                 covered=stats['primary_hits'] / stats['primary_rays'],
                 occluded_share=stats['ao_occluded'] / stats['ao_rays'] if stats['ao_rays'] else None)
        row[name] = r
    if args.only in (None, 'raycast'):
        p = FM.params(width=W, height=H, samples=ss, projection=0, **{k: tuple(float(x) for x in cam[k]) for k in ('eye', 'right', 'up', 'forward')},
                      tan_half_w=cam['tan_half_w'], tan_half_h=cam['tan_half_h'])
        rays = torch.from_numpy(FM.sample_rays(p)).to(dev)
        r = timed(lambda: mesh.raycast(rays), args.reps)
        r.update(tests=mesh.ray_tests, tests_per_ray=mesh.ray_tests / n, rays_per_second=n / (r['median_ms'] * 1e-3))
        row['raycast'] = r
    for shading in ('flat', 'smooth'):
        a, b = row.get(shading + '_k0'), row.get(shading + '_k16')
        if a and b:
            occ = b['median_ms'] - a['median_ms']
            row[shading + '_split'] = dict(occlusion_ms=occ, occlusion_rays_per_second=b['ao_rays'] / (occ * 1e-3) if occ > 0 else None,
                                           without_occlusion_ms=a['median_ms'],
                                           over_raycast_ms=a['median_ms'] - row['raycast']['median_ms'] if 'raycast' in row else None)
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
