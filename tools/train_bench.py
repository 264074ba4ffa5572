"""Time one training step of p2s_max on the device at the reference's batch (1001 items, 300-point patches, 1000-point
sub-samples) and, next to it, the float32 autograd step of the restatement (tests/train_model.py) on the same GPU through
torch-ROCm -- what the reference itself would run there.  Prints one JSON line.

    python tools/train_bench.py [--batch 1001] [--points 300] [--sub 1000] [--steps 5] [--warmup 2] [--no-torch]
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
sys.path.insert(0, os.path.join(REPO, 'tests'))


def step_flop(shapes, B, P, S):
    """algorithmic FLOP of one step: 2 M K N per linear layer forward, twice that backward (dX and dW; the K = 3 input layers
    have no dX), three 64 x 64 products per point for the feature transform"""
    total = 0
    for name, shape in shapes.items():
        if not name.endswith('.weight') or len(shape) < 2:
            continue
        n, k = int(shape[0]), int(shape[1])
        head = '.fc' in name or name.startswith('fc')
        rows = B if head else B * (P if name.startswith('feat_local') else S)
        total += 2 * rows * k * n * (2 if k == 3 else 3)
    if any('stn2' in n for n in shapes):
        total += 3 * 2 * B * (P + S) * 64 * 64
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1001)
    ap.add_argument('--points', type=int, default=300)
    ap.add_argument('--sub', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-torch', action='store_true')
    opt = ap.parse_args()
    from points2surf_amd import model_spec, synth, train
    import train_model as TM
    torch.cuda.set_device(0)
    B, P, S = opt.batch, opt.points, opt.sub
    _, cfg = synth.make_weights('p2s_max')
    cfg = dict(cfg, points_per_patch=P, sub_sample_size=S)
    state = train.init_state(cfg, seed=0)
    b = TM.make_batch(B, P, S, seed=0)
    args = [torch.from_numpy(b[k]).cuda() for k in ('patch', 'sub', 'query', 'dist_abs', 'sign01', 'radius')]
    tr = train.Trainer(cfg, state)

    def device_step():
        loss = tr.forward_backward(*args)
        tr.step(0.01, 0.9)
        return loss

    for _ in range(opt.warmup):
        device_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(opt.steps):
        loss = device_step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / opt.steps
    tr.profile(True)
    device_step()
    fam = tr.profile(False)
    fam_total = sum(fam.values())
    flop = step_flop(model_spec.state_shapes(use_feat_stn=True), B, P, S)
    out = dict(model='p2s_max', batch=B, points_per_patch=P, sub_sample_size=S, steps=opt.steps, warmup=opt.warmup,
               ms_per_step=round(ms, 3), flop_per_step=flop, tflops=round(flop / ms / 1e9, 3),
               family_share={k: round(v / fam_total, 4) for k, v in fam.items()}, family_ms_profiled=fam,
               resident_bytes=tr.resident_bytes(), last_losses=loss)
    tr.close()
    if not opt.no_torch:
        torch.cuda.empty_cache()
        m = TM.TrainModel(state, cfg, dtype=torch.float32, device='cuda', record=False)

        def torch_step():
            m.forward_backward(*args)
            m.step(0.01, 0.9)

        for _ in range(opt.warmup):
            torch_step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(opt.steps):
            torch_step()
        torch.cuda.synchronize()
        out['torch_rocm_ms_per_step'] = round((time.perf_counter() - t0) * 1e3 / opt.steps, 3)
        out['torch_rocm_peak_bytes'] = int(torch.cuda.max_memory_allocated())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
