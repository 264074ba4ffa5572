"""Time the assembly of training batches (points2surf_amd/train.py, TrainData.assemble) with both loaders on a synthetic
data set: 'per_shape' (one upload, kNN call and sub-sample call per shape of the batch) against 'set' (one of each per
batch, engine.CloudSet).  The data set has the SHAPE COUNT that decides the cost -- every batch of an epoch touches about
as many shapes as it has items -- not the reference's point counts.  Prints one JSON line.

    python tools/train_loader_bench.py [--shapes 512] [--points 20000] [--queries 1000] [--batch 501] [--patch 300]
                                       [--sub 1000] [--steps 10] [--warmup 2] [--rounds 3]

Every timed window assembles --steps batches and ends in torch.cuda.synchronize(); the two loaders alternate --rounds
times in one process and the median window is reported beside all of them.  Before timing, one batch is assembled with both
loaders from twin generators and compared byte for byte.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LOADERS = ('per_shape', 'set')


def make_data(n_shapes, n_points, n_queries, P, S, dev):
    from points2surf_amd import engine, synth, train
    rs = np.random.default_rng(0)
    names, clouds, queries, dists = [], [], [], []
    for i in range(n_shapes):
        pts = synth.make_cloud(n_points, seed=i, kind='sphere' if i % 2 else 'blob')
        names.append('shape%04d' % i)
        clouds.append(engine.Cloud(pts, dev))
        queries.append((pts[rs.integers(0, n_points, n_queries)] + rs.normal(0, 0.02, (n_queries, 3))).astype(np.float32))
        dists.append(rs.normal(0, 0.02, n_queries).astype(np.float32))
    return train.TrainData(names, clouds, queries, dists, P, S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=int, default=512)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--queries', type=int, default=1000, help='query points per shape (all of them enter an epoch)')
    ap.add_argument('--batch', type=int, default=501)
    ap.add_argument('--patch', type=int, default=300)
    ap.add_argument('--sub', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    opt = ap.parse_args()
    from points2surf_amd import engine, train
    if not torch.cuda.is_available():
        raise RuntimeError('train_loader_bench needs a ROCm GPU (gfx950): nothing is timed on the CPU')
    dev = engine.select_device(0)
    t0 = time.perf_counter()
    data = make_data(opt.shapes, opt.points, opt.queries, opt.patch, opt.sub, dev)
    setup_s = time.perf_counter() - t0
    order = train.epoch_order(data.n_queries, opt.queries, seed=1, epoch=0)
    per_window = opt.steps
    need = (opt.warmup + opt.rounds * per_window) * opt.batch
    if order.shape[0] < need:
        raise ValueError('the epoch has %d items, the run needs %d: more --shapes or --queries' % (order.shape[0], need))
    batches = [order[i * opt.batch:(i + 1) * opt.batch] for i in range(need // opt.batch)]
    distinct = [int(np.unique(b[:, 0]).size) for b in batches]

    # both loaders give the same bytes and leave the generator in the same state
    twins = [engine.Rng(7, dev) for _ in LOADERS]
    got = [data.assemble(batches[0], l, r) for l, r in zip(LOADERS, twins)]
    (mt_a, pos_a), (mt_b, pos_b) = [r.get_state() for r in twins]
    equal = all(torch.equal(a, b) for a, b in zip(*got)) and np.array_equal(mt_a, mt_b) and pos_a == pos_b
    for r in twins:
        r.close()
    if not equal:
        raise RuntimeError('the two loaders assembled different batches')

    rngs = {l: engine.Rng(11, dev) for l in LOADERS}
    for l in LOADERS:
        for b in batches[:opt.warmup]:
            data.assemble(b, l, rngs[l])
    windows = {l: [] for l in LOADERS}
    at = opt.warmup
    for _ in range(opt.rounds):
        for l in LOADERS:                                    # the same batches for both loaders of a round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in batches[at:at + per_window]:
                out = data.assemble(b, l, rngs[l])
            torch.cuda.synchronize()
            windows[l].append((time.perf_counter() - t0) * 1e3 / per_window)
            del out
        at += per_window
    res = dict(shapes=opt.shapes, points_per_cloud=opt.points, batch=opt.batch, points_per_patch=opt.patch,
               sub_sample_size=opt.sub, steps=opt.steps, warmup=opt.warmup, rounds=opt.rounds,
               distinct_shapes_per_batch=round(float(np.mean(distinct)), 1), equal_bytes=bool(equal),
               words_per_batch_estimate=int(opt.batch * opt.sub * (1 << int(opt.points - 1).bit_length()) / opt.points),
               setup_seconds=round(setup_s, 2))
    for l in LOADERS:
        res[l + '_ms_per_batch'] = round(float(np.median(windows[l])), 3)
        res[l + '_ms_windows'] = [round(w, 3) for w in windows[l]]
    res['speedup'] = round(res['per_shape_ms_per_batch'] / res['set_ms_per_batch'], 2)
    for r in rngs.values():
        r.close()
    data.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
