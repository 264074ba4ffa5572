"""Golden maker for the training step: the UNMODIFIED reference model in ``.train()`` mode, its ``compute_loss`` and two
``torch.optim.SGD`` steps on seeded synthetic weights (B = 4, P = 20, S = 30), for p2s_max and p2s_max_no_feat_stn.

Writes tests/golden/train_step_<cfg>.npz: the inputs, the losses of both steps, and per tensor the norms of the second
step's gradient and of the parameters after it, with all values of tensors below 4,096 elements and 1,024 seeded sample
positions of every larger one (tests/train_model.py ``golden_view``), and the indices its max-pools picked.  Data only.  Needs the reference tree
(oracle/ref_shims.py); run from the repository root:  python tools/make_golden_train.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

LR, MOMENTUM, STEPS = 0.01, 0.9, 2
B, P, S = 4, 20, 30


def run(name):
    from oracle import ref_shims
    from points2surf_amd import synth
    import train_model as TM
    w, cfg = synth.make_weights(name)
    batch = TM.make_batch(B, P, S, seed=7)
    with ref_shims.reference():
        from source import points_to_surf_model as ref_model
        if 'torch.utils.tensorboard' not in sys.modules:
            # the train script imports SummaryWriter at module level; compute_loss never touches it
            import types
            tb = types.ModuleType('torch.utils.tensorboard')
            tb.SummaryWriter = object
            sys.modules['torch.utils.tensorboard'] = tb
        from source import points_to_surf_train as ref_train
        torch.manual_seed(0)
        net = ref_model.PointsToSurfModel(
            net_size_max=1024, num_points=P, output_dim=2, use_point_stn=False, use_feat_stn=bool(cfg['use_feat_stn']),
            sym_op='max', use_query_point=True, sub_sample_size=S, do_augmentation=False, single_transformer=False,
            shared_transformation=False)
        net.load_state_dict(synth.to_torch_state_dict(w, module_prefix=False))
        net.train()
        opt = torch.optim.SGD(net.parameters(), lr=LR, momentum=MOMENTUM)
        out = {k: v for k, v in batch.items()}
        losses = []
        # the indices the reference's own max-pools picked (lowest index on ties, as MaxPool1d does): near-ties resolve
        # differently in float64, so the test differentiates the function the reference differentiated
        picked = {}
        for pool in TM.pool_names(cfg):
            def hook(mod, inp, outp, pool=pool):
                idx = torch.nn.functional.max_pool1d(inp[0].detach(), inp[0].shape[2], return_indices=True)[1]
                picked[pool] = idx.squeeze(2).numpy().astype(np.int16)
            net.get_submodule(pool).mp1.register_forward_hook(hook)
        for step in range(STEPS):
            opt.zero_grad()
            # the reference's forward and compute_loss write into their inputs (sub-sample -= query, target /= radius)
            data = {'patch_pts_ps': torch.from_numpy(batch['patch'].copy()),
                    'pts_sub_sample_ms': torch.from_numpy(batch['sub'].copy()),
                    'imp_surf_query_point_ms': torch.from_numpy(batch['query'].copy()),
                    'imp_surf_magnitude_ms': torch.from_numpy(batch['dist_abs'].copy()),
                    'imp_surf_dist_sign_ms': torch.from_numpy(batch['sign01'].copy()),
                    'patch_radius_ms': torch.from_numpy(batch['radius'].copy())}
            pred = net(data)
            loss = ref_train.compute_loss(pred=pred, batch_data=data, outputs=['imp_surf_magnitude', 'imp_surf_sign'],
                                          output_loss_weights={'imp_surf_magnitude': 1.0, 'imp_surf_sign': 1.0},
                                          fixed_radius=False)
            losses.append([float(loss[0].detach()), float(loss[1].detach())])
            for pool, idx in picked.items():
                out['pool/%d/%s' % (step, pool)] = idx
            sum(loss).backward()
            opt.step()
        out['losses'] = np.asarray(losses, np.float64)
        grads = {k: p.grad.detach().numpy() for k, p in net.named_parameters()}
        for k, v in net.state_dict().items():
            v = v.detach().numpy()
            if k.endswith('num_batches_tracked'):
                out['state/' + k] = v.astype(np.int64)
                continue
            out['state/' + k] = TM.golden_view(v).astype(np.float32)
            out['state_norm/' + k] = np.float64(np.linalg.norm(v.astype(np.float64)))
            if k in grads:
                out['grad/' + k] = TM.golden_view(grads[k]).astype(np.float32)
                out['grad_norm/' + k] = np.float64(np.linalg.norm(grads[k].astype(np.float64)))
    path = os.path.join(REPO, 'tests', 'golden', 'train_step_%s.npz' % name)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes, losses', losses)


if __name__ == '__main__':
    for n in ('p2s_max', 'p2s_max_no_feat_stn'):
        run(n)
