"""TEST INFRASTRUCTURE ONLY -- goldens of the reference's multi-worker sub-sample streams (``--workers W
--batchSize B``), from the UNMODIFIED reference.  Run in the build container only (needs a reference checkout):

    python tools/make_golden_workers.py <case> [<case> ...]     # one case per process; cases run side by side
    python tools/make_golden_workers.py merge                   # meta of every finished case -> meta_workers.json

Why: every eval script the reference ships runs with ``--batchSize 501 --workers 7``.  torch's map-style DataLoader
hands batch b (positions [b B, (b+1) B) of the sampler's sequence, across shapes) to worker b mod W, and every worker
holds its own copy of the dataset -- so of both ``np.random.RandomState(seed)`` objects (source/data_loader.py:270-277).
Query g therefore draws from worker stream (g // B) mod W.

Per case:
  * the reference's ``points_to_surf_eval(opt)`` with ``--workers W --batchSize B``: ``rec/dist_ms`` of every shape
    (the GT-query pass: ``eval/eval``; the random-patch sampler: also ``rec/<shape>.idx``);
  * ``make_dataset`` + ``make_datasampler`` + ``make_dataloader`` with the same W and B, no network: per batch the
    sha256 of ``pts_sub_sample_ms``, ``patch_pts_ps`` and ``patch_radius_ms`` exactly as they arrive (float32);
  * self-check (recorded in the meta): every batch's sub-sample rebuilt from W ``RandomState(seed)`` copies serving the
    batches round-robin, through numpy's generator and the reference's own ``get_point_cloud_sub_sample`` (+ the
    rotation of the GT-query pass from W twins of the first generator); every digest must match.

Output: tests/golden/ref_workers_<case>.npz + entries in tests/golden/meta_workers.json.  Weights: seeded synthetic
(points2surf_amd/synth.py, seed 1234) like every other golden.  Data seed: the reference default (40938661).
"""
import copy
import glob
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from oracle import ref_shims  # noqa: E402
from oracle.make_golden import train_namespace, sha, SEED_DATA  # noqa: E402
from oracle import make_golden_sizes as sizes  # noqa: E402
from points2surf_amd import synth  # noqa: E402

PATCHES_PER_SHAPE = 1000       # random-patch case: 3 x 1000 of the sampler's picks, 82 batches of 37

# name -> (model, workers, batch, pass): 'rec' reconstruction at grid 32, 'gt' the GT-query pass (05_query_pts),
# 'recsample' reconstruction with --sampling sequential_shapes_random_patches
CASES = {
    'p2s_max_w7_b501': ('p2s_max', 7, 501, 'rec'),
    'p2s_vanilla_w7_b501': ('p2s_vanilla', 7, 501, 'rec'),
    'p2s_max_w3_b37': ('p2s_max', 3, 37, 'rec'),
    'p2s_vanilla_w3_b37': ('p2s_vanilla', 3, 37, 'rec'),
    'p2s_medium_radius_w7_b501': ('p2s_medium_radius', 7, 501, 'rec'),
    'p2s_max_w7_b501_gt': ('p2s_max', 7, 501, 'gt'),
    'p2s_max_w3_b37_recsample': ('p2s_max', 3, 37, 'recsample'),
}
RES = 32
META_TMP = os.path.join(sizes.GOLDEN, '.workers_meta_%s.json')


def _digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy(), dtype=np.float32).tobytes()).digest()


def run(case):
    import torch
    model, W, B, kind = CASES[case]
    torch.set_num_threads(int(os.environ.get('P2S_GOLDEN_THREADS', 2)))
    ref_shims.install()
    from source import points_to_surf_eval as ref_eval
    from source.base import utils as ref_utils
    import trimesh
    w, cfg = synth.make_weights(model, seed=1234)
    tmp = tempfile.mkdtemp(prefix='p2s_golden_w_')
    out = {}
    meta = {'model': model, 'dataset': 'abc3', 'grid': RES, 'job': 'workers', 'pass': kind, 'workers': W, 'batchSize': B,
            'seed': SEED_DATA, 'torch': torch.__version__, 'numpy': np.__version__}
    try:
        modeldir = os.path.join(tmp, 'models')
        os.makedirs(modeldir)
        torch.save(synth.to_torch_state_dict(w), os.path.join(modeldir, model + '_model.pth'))
        train_opt = train_namespace(cfg, batch=500)
        torch.save(train_opt, os.path.join(modeldir, model + '_params.pth'))
        indir = os.path.join(sizes.dataset_dir(tmp), 'abc_minimal')
        outdir = os.path.join(tmp, 'out')
        args = ['--indir', indir, '--outdir', outdir, '--dataset', 'abc3.txt', '--modeldir', modeldir, '--models', model,
                '--query_grid_resolution', str(RES), '--epsilon', '3', '--certainty_threshold', '13', '--sigma', '5',
                '--gpu_idx', '-1', '--workers', str(W), '--batchSize', str(B), '--cache_capacity', '5']
        if kind == 'recsample':
            args += ['--sampling', 'sequential_shapes_random_patches', '--patches_per_shape', str(PATCHES_PER_SHAPE)]
            meta['patches_per_shape'] = PATCHES_PER_SHAPE
        names = sizes.shapes_of('abc3')

        # ---- 1. the data path alone: the batches as the workers deliver them ----
        opt = ref_eval.parse_arguments(args)
        opt.reconstruction = kind != 'gt'
        dataset = ref_eval.make_dataset(train_opt=train_opt, eval_opt=opt)
        pristine = copy.deepcopy(dataset)           # what every worker starts from
        sampler = ref_eval.make_datasampler(eval_opt=opt, dataset=dataset)
        loader = ref_eval.make_dataloader(eval_opt=opt, dataset=dataset, datasampler=sampler, model_batch_size=B)
        h_sub, h_patch, h_rad, sizes_b = [], [], [], []
        for batch in loader:
            h_sub.append(_digest(batch['pts_sub_sample_ms']))
            h_patch.append(_digest(batch['patch_pts_ps']))
            h_rad.append(_digest(batch['patch_radius_ms']))
            sizes_b.append(int(batch['pts_sub_sample_ms'].shape[0]))
        out['sub_sha'] = np.frombuffer(b''.join(h_sub), np.uint8).reshape(-1, 32)
        out['patch_sha'] = np.frombuffer(b''.join(h_patch), np.uint8).reshape(-1, 32)
        out['radius_sha'] = np.frombuffer(b''.join(h_rad), np.uint8).reshape(-1, 32)
        out['batch_sizes'] = np.asarray(sizes_b, np.int32)
        meta['batches'] = len(sizes_b)

        # ---- 2. self-check: the stream model, through numpy's own generator ----
        order = list(iter(ref_eval.make_datasampler(eval_opt=opt, dataset=pristine)))   # a fresh sampler: same picks
        assert len(order) == sum(sizes_b)
        out['positions'] = np.asarray(order, np.int64) if kind == 'recsample' else np.zeros(0, np.int64)
        shapes = [pristine.shape_cache.get(s) for s in range(len(names))]
        offs = np.concatenate([[0], np.cumsum(pristine.shape_patch_count)])
        sub_rng = [np.random.RandomState(SEED_DATA) for _ in range(W)]
        rot_rng = [np.random.RandomState(SEED_DATA) for _ in range(W)]
        uniform = bool(train_opt.uniform_subsample)
        ok = 0
        for b, size in enumerate(sizes_b):
            wk = b % W
            pts = []
            for g in order[b * B:b * B + size]:
                s = int(np.searchsorted(offs, g, side='right') - 1)
                qp = shapes[s].imp_surf_query_point_ms[g - offs[s]]
                p = ref_utils.get_point_cloud_sub_sample(sub_sample_size=train_opt.sub_sample_size, pts_ms=shapes[s].pts,
                                                         query_point_ms=qp, rng=sub_rng[wk], uniform=uniform, fixed=False)
                if kind == 'gt':
                    rot = trimesh.transformations.random_rotation_matrix(rot_rng[wk].rand(3))
                    p = trimesh.transformations.transform_points(p, rot).astype(np.float32)
                pts.append(np.asarray(p, np.float32))
            got = hashlib.sha256(np.ascontiguousarray(np.stack(pts), dtype=np.float32).tobytes()).digest()
            assert got == h_sub[b], 'batch %d (worker %d): the stream model does not reproduce the reference' % (b, wk)
            ok += 1
        meta['self_check'] = {'batches_rebuilt': ok, 'model': 'query g draws from RandomState(seed) copy (g // B) mod W'}
        # ---- 3. the reference's own eval with the workers ----
        opt = ref_eval.parse_arguments(args)
        opt.reconstruction = kind != 'gt'
        t0 = time.time()
        ref_eval.points_to_surf_eval(opt)
        meta['reference_seconds'] = time.time() - t0
        meta['shapes'] = []
        for i, n in enumerate(names):
            if kind == 'gt':
                d = np.load(os.path.join(outdir, 'eval', 'eval', n + '.xyz.npy')).astype(np.float32)
            else:
                d = np.load(os.path.join(outdir, 'rec', 'dist_ms', n + '.xyz.npy')).astype(np.float32)
                q = np.load(os.path.join(outdir, 'rec', 'query_pts_ms', n + '.xyz.npy'))
            out['sdf_%d' % i] = d
            sh = {'name': n, 'queries': int(d.shape[0]), 'pos_frac': float((d > 0).mean())}
            if kind != 'gt':
                sh['query_sha256'] = sha(q)
            if kind == 'recsample':
                out['idx_%d' % i] = np.loadtxt(os.path.join(outdir, 'rec', n + '.idx'), dtype=np.int64).astype(np.int32)
            meta['shapes'].append(sh)
        meta['queries_total'] = int(sum(s['queries'] for s in meta['shapes']))
        meta['reference_queries_per_s'] = meta['queries_total'] / meta['reference_seconds']

    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    key = 'ref_workers_' + case
    np.savez_compressed(os.path.join(sizes.GOLDEN, key + '.npz'), **out)
    with open(META_TMP % case, 'w') as f:
        json.dump(meta, f)
    print(key, json.dumps(meta), flush=True)


def merge():
    """the meta of every finished case into tests/golden/meta_workers.json (the goldens of this script keep a meta file
    of their own; the other generators' meta files stay untouched)"""
    path = os.path.join(sizes.GOLDEN, 'meta_workers.json')
    meta = {}
    if os.path.isfile(path):
        with open(path) as f:
            meta = json.load(f)
    done = sorted(glob.glob(META_TMP % '*'))
    for p in done:
        case = os.path.basename(p)[len('.workers_meta_'):-len('.json')]
        with open(p) as f:
            meta['ref_workers_' + case] = json.load(f)
    with open(path, 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    for p in done:
        os.remove(p)


if __name__ == '__main__':
    if sys.argv[1:] == ['merge']:
        merge()
    else:
        for c in sys.argv[1:] or sorted(CASES):
            run(c)
