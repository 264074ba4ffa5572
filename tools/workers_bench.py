"""Throughput of workers mode (the reference's ``--workers 7 --batchSize 501`` sub-sample streams) next to the default
dataset mode (one stream, ``--workers 0``), in one process on one GPU.  bench.py is not involved.

    python tools/workers_bench.py [--steps 3] [--warmup 1] [--workers 7] [--batch 501] [--res 256] [--out FILE]

Workload per step: the three abc3 clouds at ``--res`` (bench.py's default dataset), each shape host to host with a fresh
cloud handle, fp32 encoders, one generator set carried across shapes and steps.  Steps of the two modes alternate, so
drift hits both alike.  Prints one JSON line per model: both rates (queries/s, median over the timed steps), their
ratio, and the device memory the W-stream generator set holds (free-memory drop over its creation and first step,
next to the same for the one dataset-mode generator).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ABC = os.path.join(REPO, 'tests', 'golden', 'abc_minimal')
SEED = 40938661
EPSILON = 3


def shapes():
    with open(os.path.join(ABC, 'abc3.txt')) as f:
        names = [x.strip() for x in f if x.strip()]
    return [np.ascontiguousarray(np.load(os.path.join(ABC, '04_pts', n + '.xyz.npy'))[:, :3], dtype=np.float32) for n in names]


def step(engine, model, clouds, gen, res):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nq = 0
    for pts in clouds:
        c = engine.Cloud(pts)
        sdf, _ = engine.infer_shape(model, c, gen, res, EPSILON, want_queries=False)
        nq += int(sdf.cpu().shape[0])
        c.close()
    return nq, time.perf_counter() - t0


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def run_model(engine, synth, name, clouds, args):
    w, cfg = synth.make_weights(name)
    cfg = dict(cfg, encoder_bf16=0)
    model = engine.Model(w, cfg)
    f0 = free_bytes()
    rng = engine.Rng(SEED)
    step(engine, model, clouds[:1], rng, 32)
    mem_dataset = f0 - free_bytes()
    f0 = free_bytes()
    ws = engine.WorkerStreams(SEED, args.workers, args.batch)
    step(engine, model, clouds[:1], ws, 32)
    mem_workers = f0 - free_bytes()
    rates = {'dataset': [], 'workers': []}
    for i in range(args.warmup + args.steps):
        for mode, gen in (('dataset', rng), ('workers', ws)):
            nq, dt = step(engine, model, clouds, gen, args.res)
            if i >= args.warmup:
                rates[mode].append(nq / dt)
    rd, rw = float(np.median(rates['dataset'])), float(np.median(rates['workers']))
    out = {'tool': 'workers_bench', 'model': name, 'encoder': 'fp32', 'grid': args.res, 'dataset': 'abc3',
           'workers': args.workers, 'batchSize': args.batch, 'steps': args.steps, 'warmup': args.warmup,
           'dataset_queries_per_s': round(rd, 1), 'workers_queries_per_s': round(rw, 1), 'ratio': round(rw / rd, 4),
           'dataset_steps': [round(r, 1) for r in rates['dataset']], 'workers_steps': [round(r, 1) for r in rates['workers']],
           'generator_set_bytes': int(mem_workers), 'dataset_generator_bytes': int(mem_dataset)}
    ws.close()
    rng.close()
    model.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--workers', type=int, default=7)
    ap.add_argument('--batch', type=int, default=501)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--models', default='p2s_max,p2s_vanilla')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    from points2surf_amd import engine, synth
    engine.select_device(0)
    clouds = shapes()
    for name in args.models.split(','):
        line = json.dumps(run_model(engine, synth, name, clouds, args))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
