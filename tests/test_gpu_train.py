"""The device training step (points2surf_amd/train.py, csrc/p2s_train.hip) against the float64 restatement of the
reference's train-mode step (tests/train_model.py), net size 1024, both trainable configurations.

Shapes (B, P, S): (5, 37, 53) nothing is a multiple of a 64-row tile (item 0 padded with duplicate points: exact pool
ties); (3, 64, 33) exactly one row tile per patch beside partial ones; (2, 8, 8) the smallest legal batch; (33, 64, 70)
M = 2112 and 2310 point rows: the weight gradients of the point-wise layers are summed over two 2048-row slabs, one of them
exactly full and one partial; (2049, 2, 3) M = 4098 and 6147 (3 and 4 slabs), M = B = 2049 in the per-item layers (two slabs,
the 4096 x 256 partials of the arena) and a loss summed over more than one pass of its 256 threads.

GRADIENTS.  Per parameter tensor ||g_dev - g_cpu||_2 / ||g_cpu||_2 against the float64 restatement with every max-pool
forced to the DEVICE's recorded indices.  The gate is measured, not fixed: the same restatement runs in float32 on the
CPU with the same forced indices, and the gate is 4x its largest per-tensor distance from the float64 run on these inputs
(the device sums in another order).  Biases whose gradient is zero in exact arithmetic (train_model.zero_grad_names) are
compared absolutely: ||g_dev||_2 <= gate * ||dW_cpu||_2 of the same layer; exact zeros are allowed.  Parameters and
running statistics after SGD steps follow the same rule.  Losses: train_model.loss_gates (the measured float32 logit
error times the losses' Lipschitz constants).

POOL INDICES.  Where the device's index differs from the float64 argmax, the float64 value at the device's index must lie
within fp32 rounding of the maximum: the pooled tensor is at most 12 linear layers of K <= 128 products deep (batch-norm
keeps every layer O(1)), so |z_max - z_dev| <= 12 * 128 * 2^-24 * max|z| of that channel = 9.2e-5 of the channel's
largest magnitude; a wrong pick is off by O(0.1) of it.  At most 0.1 % of all (item, channel) pairs may differ at all; the
seeds are chosen so that float32-CPU against float64-CPU stays under 0.025 % on the same inputs, which is checked here.

RELU MASKS.  A ReLU is the other place where two precisions can differentiate different pieces of the network: a unit whose
pre-activation lies within fp32 rounding of zero is let through by one and not by the other, which moves a gradient by
about 1 / sqrt(active units).  At (2049, 2, 3) the step has 21.8 M such units and a tie is the expected case: measured on the
MI355X with p2s_max, three units whose float64 pre-activations lie within 3e-8 of their channel's largest magnitude are
masked the other way by the device; left to the float64 signs, 52 of 76 gradient tensors miss the 7.8e-6 gate (worst
1.1e-3), and with the device's masks all agree within 1.64e-6.  So the CPU runs of _one_step take the DEVICE's masks
(p2s_debug_train_relu_masks) as they take its pool indices, in both precisions, and test_relu_masks holds the device to
them: where its mask differs from the sign of the float64 pre-activation, that pre-activation must lie within fp32 rounding
of zero.  The bound follows the pool rule: a unit lies behind at most 15 linear layers whose reduced lengths add up to
3 + 3 x 64 + 128 + 1024 + 512 + 256 + 3 x 64 + 128 + 1024 + 1024 + 256 = 4739 products (batch-norm keeps every layer
O(1)), so |z| <= 4739 * 2^-24 * max|z| of its channel = 2.8e-4 of the channel's largest magnitude, and at most 0.1 % of all
units may differ at all.  A mask that is wrong by more than rounding fails this rule; a right one leaves the gates what they
were: 4x the float32-CPU error, the loss gates and the pool rule unchanged.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import train_model as TM  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = ['p2s_max', 'p2s_max_no_feat_stn']
SHAPES = [(5, 37, 53, True), (3, 64, 33, False), (2, 8, 8, False), (33, 64, 70, False), (2049, 2, 3, False)]
SLAB_SHAPE = SHAPES[3]
SEED = 1
POOL_ROUNDING = 12 * 128 * 2.0 ** -24
RELU_ROUNDING = 4739 * 2.0 ** -24
GATE_FACTOR = 4.0


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    torch.cuda.set_device(0)
    return torch


def _weights(name, P, S):
    from points2surf_amd import synth
    w, cfg = synth.make_weights(name)
    return w, dict(cfg, points_per_patch=P, sub_sample_size=S)


def _dev_batch(torch, b):
    return [torch.from_numpy(b[k]).cuda() for k in ('patch', 'sub', 'query', 'dist_abs', 'sign01', 'radius')]


def _cpu_args(b):
    return [b[k] for k in ('patch', 'sub', 'query', 'dist_abs', 'sign01', 'radius')]


def _gate(t32, t64, skip=()):
    return GATE_FACTOR * max(TM.rel_err(t32[k], v) for k, v in t64.items() if k not in skip and np.ndim(v) > 0)


def _check_tensors(dev, ref, gate, what, zero=(), ref_grads=None):
    worst = 0.0
    for k, v in ref.items():
        if np.ndim(v) == 0:
            continue
        if k in zero:
            wn = np.linalg.norm(ref_grads[k[:-4] + 'weight'])
            assert np.linalg.norm(dev[k]) <= gate * wn, (what, k, np.linalg.norm(dev[k]), gate * wn)
            continue
        e = TM.rel_err(dev[k], v)
        worst = max(worst, e)
        assert e <= gate, (what, k, e, gate)
    return worst


def _relu_masks(tr, cfg, B, P, S):
    """the device's ReLU masks of the last step, one array per ReLU of train_model's forward, shaped like its input"""
    import ctypes
    from points2surf_amd import _lib
    layers = []                         # (points per item or 0 for a per-item layer, channels), in forward order
    for pts in (S, P):
        layers += [(pts, 64), (pts, 64)]
        if cfg.get('use_feat_stn', True):
            layers += [(pts, 64), (pts, 128), (pts, 1024), (0, 512), (0, 256)]
        layers += [(pts, 64), (pts, 128), (0, 512)]
    layers += [(0, 256), (0, 128)]
    flat = np.empty(sum(B * max(pts, 1) * C for pts, C in layers), np.uint8)
    _lib.check(tr.lib.p2s_debug_train_relu_masks(tr.handle, flat.ctypes.data_as(ctypes.c_void_p), flat.size))
    assert flat.max() <= 1
    out, o = [], 0
    for pts, C in layers:
        n = B * max(pts, 1) * C
        m = flat[o:o + n]
        out.append(np.ascontiguousarray(m.reshape(B, pts, C).transpose(0, 2, 1)) if pts else m.reshape(B, C))
        o += n
    return out


_step_cache = {}


def _one_step(torch, name, shape):
    """device step + the CPU runs every test of this (configuration, shape) shares; computed once, never modified"""
    key = (name, shape)
    if key in _step_cache:
        return _step_cache[key]
    import torch as th
    from points2surf_amd import train
    B, P, S, pad = shape
    w, cfg = _weights(name, P, S)
    b = TM.make_batch(B, P, S, SEED, pad)
    tr = train.Trainer(cfg, w)
    loss = tr.forward_backward(*_dev_batch(torch, b))
    r = dict(batch=b, cfg=cfg, w=w, loss=loss, grads=tr.grads(), pools=tr.pool_indices(), state=tr.state_dict(module_prefix=False),
             relu=_relu_masks(tr, cfg, B, P, S))
    tr.close()
    free64 = TM.TrainModel(w, cfg)
    free64.forward_backward(*_cpu_args(b))
    r['free64_pools'], r['free64_inputs'] = free64.pools, free64.pool_inputs
    free32 = TM.TrainModel(w, cfg, dtype=th.float32)
    free32.forward_backward(*_cpu_args(b))
    r['free32_pools'] = free32.pools
    for tag, dt in (('f64', th.float64), ('f32', th.float32)):
        m = TM.TrainModel(w, cfg, dtype=dt)
        r[tag + '_loss'] = m.forward_backward(*_cpu_args(b), forced=r['pools'], forced_relu=r['relu'])
        r[tag + '_grads'], r[tag + '_state'], r[tag + '_pred'] = m.grads(), m.state(), m.pred
        r[tag + '_relu_ties'], r[tag + '_relu_units'] = m.relu_ties, m.relu_units
    _step_cache[key] = r
    return r


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s[:3])
@pytest.mark.parametrize('name', CONFIGS)
def test_losses_and_gradients(name, shape, torch_cuda):
    r = _one_step(torch_cuda, name, shape)
    zero = TM.zero_grad_names(r['f64_grads'])
    gate = _gate(r['f32_grads'], r['f64_grads'], skip=zero)
    loss_gate = TM.loss_gates(r['f32_pred'], r['f64_pred'], r['f64_loss'], GATE_FACTOR)
    print('%s %s: losses device %s float64 %s (gates %s); gradient gate %.3g' % (name, shape[:3], r['loss'], r['f64_loss'],
                                                                                 loss_gate, gate))
    for a, b, t in zip(r['loss'], r['f64_loss'], loss_gate):
        assert abs(a - b) <= t, (r['loss'], r['f64_loss'], loss_gate)
    assert set(r['grads']) == set(r['f64_grads'])
    worst = _check_tensors(r['grads'], r['f64_grads'], gate, 'gradient', zero=zero, ref_grads=r['f64_grads'])
    print('%s %s: worst device gradient error %.3g, float32-CPU gate (4x) %.3g' % (name, shape[:3], worst, gate))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s[:3])
@pytest.mark.parametrize('name', CONFIGS)
def test_pool_indices(name, shape, torch_cuda):
    r = _one_step(torch_cuda, name, shape)
    B, P, S, pad = shape
    assert list(r['pools']) == list(TM.pool_names(r['cfg']))
    n = differ = differ32 = 0
    for pool, idx in r['pools'].items():
        pts = S if pool.startswith('feat_global') else P
        assert idx.shape == (B, 1024) and idx.min() >= 0 and idx.max() < pts
        ref, z = r['free64_pools'][pool], r['free64_inputs'][pool].numpy()            # z [B, 1024, points]
        ref32 = r['free32_pools'][pool]
        if pad:
            # the padded rows of item 0 are copies of its row 0.  The device computes every row by the same sequence of
            # operations, so copies tie exactly and the lowest index wins; a CPU BLAS may round equal rows differently by
            # their place in its blocks, so on the CPU a copy can win by an ulp: count a copy as the row it copies
            assert idx[0].max() < pts // 2
            ref, ref32 = ref.copy(), ref32.copy()
            ref[0][ref[0] >= pts // 2] = 0
            ref32[0][ref32[0] >= pts // 2] = 0
        n += idx.size
        differ += int((idx != ref).sum())
        differ32 += int((ref32 != ref).sum())
        at_dev = np.take_along_axis(z, idx[:, :, None].astype(np.int64), axis=2)[:, :, 0]
        bound = POOL_ROUNDING * np.abs(z).max(axis=(0, 2))[None, :]
        assert (z.max(axis=2) - at_dev <= bound).all(), (pool, float((z.max(axis=2) - at_dev - bound).max()))
    print('%s %s: %d of %d pool picks differ from float64 (float32 CPU: %d)' % (name, shape[:3], differ, n, differ32))
    assert differ32 <= 0.00025 * n
    assert differ <= 0.001 * n


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s[:3])
@pytest.mark.parametrize('name', CONFIGS)
def test_relu_masks(name, shape, torch_cuda):
    """the device's ReLU masks against the float64 pre-activations (module docstring, RELU MASKS)"""
    r = _one_step(torch_cuda, name, shape)
    ties, n = r['f64_relu_ties'], r['f64_relu_units']
    assert len(ties) == len(r['relu']) == (22 if r['cfg'].get('use_feat_stn', True) else 12) and n == sum(m.size for m in r['relu'])
    differ = sum(t.size for t in ties)
    worst = max([float(t.max()) for t in ties if t.size] or [0.0])
    print('%s %s: %d of %d ReLU units masked unlike float64 (unlike float32 on the CPU: %d), the furthest from zero at %.3g of its channel'
          % (name, shape[:3], differ, n, sum(t.size for t in r['f32_relu_ties']), worst))
    assert worst <= RELU_ROUNDING, (worst, RELU_ROUNDING)
    assert differ <= 0.001 * n


def _check_running_statistics(torch_cuda, name, shape):
    r = _one_step(torch_cuda, name, shape)
    bufs = [k for k in r['f64_state'] if k.endswith(('running_mean', 'running_var'))]
    gate = _gate({k: r['f32_state'][k] for k in bufs}, {k: r['f64_state'][k] for k in bufs})
    _check_tensors({k: r['state'][k].numpy() for k in bufs}, {k: r['f64_state'][k] for k in bufs}, gate, 'buffer')
    for k, v in r['state'].items():
        if k.endswith('num_batches_tracked'):
            assert v.dtype == torch_cuda.int64 and int(v) == 1001 == int(r['f64_state'][k])


@pytest.mark.parametrize('name', CONFIGS)
def test_running_statistics_after_one_step(name, torch_cuda):
    _check_running_statistics(torch_cuda, name, SHAPES[0])


@pytest.mark.parametrize('name', CONFIGS)
def test_running_statistics_after_one_step_with_two_slabs(name, torch_cuda):
    _check_running_statistics(torch_cuda, name, SLAB_SHAPE)


@pytest.mark.parametrize('name', CONFIGS)
def test_three_sgd_steps_in_lockstep_and_round_trip(name, torch_cuda):
    """three steps, lr changed before the third; each CPU step is forced to that step's device indices.  Then the exported
    checkpoint runs through weights.build_blob / engine.Model and agrees with the CPU port on the same dict.

    Shape and batches.  Besides a max-pool a ReLU is where two precisions can differentiate different functions: a unit
    whose pre-activation lies within rounding of zero is masked in one and not in the other, which moves a gradient by
    about 1 / sqrt(active units) ~ 1 % at these sizes -- between float32 and float64 on the CPU as well, and after the next
    update the two runs drift apart.  Forcing the pool indices does not remove that, so the batches are chosen where it
    cannot happen easily: B = 8 (a batch-norm over the 5 rows of the other cases divides by the deviation of five
    numbers), few points (432k ReLU units per step), and of the seeds 100..159 the one whose float64 run on the CPU keeps
    every ReLU pre-activation of all three steps furthest from zero (seed 120: 6e-6 of the layer's deviation for p2s_max,
    8.7e-6 without feature transforms; found on the CPU alone, with batch seeds seed + 1000 * step)."""
    import torch as th
    from points2surf_amd import engine, train
    from oracle import torch_port, p2s_oracle
    B, P, S, pad, seed0 = 8, 9, 11, False, 120
    w, cfg = _weights(name, P, S)
    tr = train.Trainer(cfg, w)
    cpu = {th.float64: TM.TrainModel(w, cfg), th.float32: TM.TrainModel(w, cfg, dtype=th.float32)}
    for step, lr in enumerate((0.01, 0.01, 0.002)):
        b = TM.make_batch(B, P, S, seed0 + 1000 * step, pad)
        loss = tr.forward_backward(*_dev_batch(torch_cuda, b))
        pools = tr.pool_indices()
        ref = {dt: m.forward_backward(*_cpu_args(b), forced=pools) for dt, m in cpu.items()}
        loss_gate = TM.loss_gates(cpu[th.float32].pred, cpu[th.float64].pred, ref[th.float64], GATE_FACTOR)
        assert all(abs(a - c) <= t for a, c, t in zip(loss, ref[th.float64], loss_gate)), (step, loss, ref, loss_gate)
        tr.step(lr, 0.9)
        for m in cpu.values():
            m.step(lr, 0.9)
    sd = tr.state_dict(module_prefix=False)
    s64, s32 = cpu[th.float64].state(), cpu[th.float32].state()
    gate = _gate(s32, s64)
    worst = _check_tensors({k: v.numpy() for k, v in sd.items()}, s64, gate, 'state after three steps')
    print('%s: worst parameter / buffer error after three steps %.3g, gate %.3g' % (name, worst, gate))
    assert all(int(v) == 1003 for k, v in sd.items() if k.endswith('num_batches_tracked'))
    # round trip: the reference's key names with the DataParallel prefix, loaded like any checkpoint
    exported = tr.state_dict()
    assert all(k.startswith('module.') for k in exported)
    from points2surf_amd import model_spec
    plain = {k: v.numpy() for k, v in model_spec.strip_module_prefix(exported).items()}
    model = engine.Model(plain, cfg)
    b = TM.make_batch(7, P, S, 99)
    logits, _ = model.forward(*_dev_batch(torch_cuda, b)[:3])
    if cfg['use_feat_stn']:
        ref = torch_port.TorchPort(plain, cfg).forward(b['patch'], b['sub'], b['query']).numpy()
    else:       # the torch port always runs the feature transform; the numpy oracle is the same forward without it
        ref = p2s_oracle.model_forward(plain, cfg, b['patch'], b['sub'], b['query'])
    assert np.abs(logits.cpu().numpy() - ref).max() < 1e-4, np.abs(logits.cpu().numpy() - ref).max()
    model.close()
    tr.close()


def _check_equal_bytes(torch_cuda, name, shape):
    from points2surf_amd import train
    B, P, S, pad = shape
    w, cfg = _weights(name, P, S)
    b = TM.make_batch(B, P, S, SEED, pad)
    out = []
    for _ in range(2):
        tr = train.Trainer(cfg, w)
        for _ in range(2):
            tr.forward_backward(*_dev_batch(torch_cuda, b))
            g = tr.grads()
            tr.step(0.01, 0.9)
        out.append((g, {k: v.numpy() for k, v in tr.state_dict().items()}))
        tr.close()
    for k, v in out[0][0].items():
        assert v.tobytes() == out[1][0][k].tobytes(), k
    for k, v in out[0][1].items():
        assert v.tobytes() == out[1][1][k].tobytes(), k


@pytest.mark.parametrize('name', CONFIGS)
def test_equal_state_and_batch_give_equal_bytes(name, torch_cuda):
    _check_equal_bytes(torch_cuda, name, SHAPES[0])


@pytest.mark.parametrize('name', CONFIGS)
def test_equal_state_and_batch_give_equal_bytes_with_two_slabs(name, torch_cuda):
    """the slab partials are reduced in slab order: equal bytes through p2s_train_slab_reduce_kernel as well"""
    _check_equal_bytes(torch_cuda, name, SLAB_SHAPE)


def test_refusals(torch_cuda):
    from points2surf_amd import synth, train, _lib
    for model in ('p2s_vanilla', 'p2s_uniform', 'p2s_shared_encoder', 'p2s_max_sum', 'p2s_regression', 'p2s_small_radius'):
        _, cfg = synth.make_weights(model)
        with pytest.raises(ValueError):
            train.Trainer(cfg)
    _, cfg = synth.make_weights('p2s_max')
    with pytest.raises(ValueError, match='net size'):
        train.Trainer(dict(cfg, net_size=512))
    B, P, S, _ = SHAPES[2]
    w, cfg = _weights('p2s_max', P, S)
    tr = train.Trainer(cfg, w)
    b = TM.make_batch(B, P, S, SEED)
    one = [t[:1] for t in _dev_batch(torch_cuda, b)]
    with pytest.raises(_lib.P2SError, match='at least 2'):
        tr.forward_backward(*one)
    before = {k: v.numpy().tobytes() for k, v in tr.state_dict().items()}
    bad = dict(b, dist_abs=b['dist_abs'].copy())
    bad['dist_abs'][1] = np.nan
    with pytest.raises(_lib.P2SError, match='non-finite'):
        tr.forward_backward(*_dev_batch(torch_cuda, bad))
    with pytest.raises(_lib.P2SError, match='no gradients'):
        tr.step(0.01, 0.9)
    after = {k: v.numpy().tobytes() for k, v in tr.state_dict().items()}
    assert before == after
    tr.forward_backward(*_dev_batch(torch_cuda, b))           # and the trainer still works
    tr.step(0.01, 0.9)
    tr.close()


@pytest.mark.parametrize('name', CONFIGS)
def test_overfits_one_batch(name, torch_cuda):
    """20 steps on one fixed batch, lr 0.01, momentum 0.9: the total loss falls below 0.7x its initial value -- asserted for
    the device only after the float64 restatement has done so on this batch"""
    from points2surf_amd import train
    B, P, S = 8, 16, 24
    w, cfg = _weights(name, P, S)
    b = TM.make_batch(B, P, S, 11)
    cpu, ref = TM.TrainModel(w, cfg), []
    for _ in range(20):
        ref.append(sum(cpu.forward_backward(*_cpu_args(b))))
        cpu.step(0.01, 0.9)
    assert ref[-1] < 0.7 * ref[0], ref
    tr, dev = train.Trainer(cfg, w), []
    args = _dev_batch(torch_cuda, b)
    for _ in range(20):
        dev.append(sum(tr.forward_backward(*args)))
        tr.step(0.01, 0.9)
    tr.close()
    print('%s: total loss %.4f -> %.4f on the device, %.4f -> %.4f in float64' % (name, dev[0], dev[-1], ref[0], ref[-1]))
    assert dev[-1] < 0.7 * dev[0], dev


def test_command_line_trains_and_the_result_loads(tmp_path, torch_cuda):
    """two synthetic shapes, two epochs; both files are written and load through the path the evaluation uses"""
    from points2surf_amd import engine, synth
    from points2surf_amd.dropin.source import points_to_surf_eval as ev
    root = str(tmp_path / 'data')
    names = synth.make_standin_dataset(root, [synth.make_cloud(3000, seed=0), synth.make_cloud(3000, seed=1, kind='sphere')], 2,
                                       list_name='trainset.txt')
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, '05_query_pts'))
    os.makedirs(os.path.join(root, '05_query_dist'))
    for n in names:
        pts = np.load(os.path.join(root, '04_pts', n + '.xyz.npy'))
        q = (pts[rng.integers(0, pts.shape[0], 40)] + rng.normal(0, 0.02, (40, 3))).astype(np.float32)
        np.save(os.path.join(root, '05_query_pts', n + '.ply.npy'), q)
        np.save(os.path.join(root, '05_query_dist', n + '.ply.npy'), rng.normal(0, 0.02, 40).astype(np.float32))
    out = str(tmp_path / 'models')
    cmd = [sys.executable, '-m', 'points2surf_amd.train', '--indir', root, '--name', 'tiny', '--outdir', out, '--nepoch', '2',
           '--batchSize', '8', '--patches_per_shape', '16', '--points_per_patch', '32', '--sub_sample_size', '64',
           '--scheduler_steps', '1', '--seed', '3']
    res = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count('epoch') == 2 and 'lr 0.001' in res.stdout, res.stdout
    model_file, params_file = os.path.join(out, 'tiny_model.pth'), os.path.join(out, 'tiny_params.pth')
    assert os.path.isfile(model_file) and os.path.isfile(params_file)
    train_opt = ev._load_train_opt(params_file)
    cfg = ev._engine_cfg(train_opt, ev.get_output_dimensions(train_opt))
    assert cfg['points_per_patch'] == 32 and cfg['sub_sample_size'] == 64 and cfg['use_feat_stn'] and cfg['uniform_subsample']
    sd = torch_cuda.load(model_file, map_location='cpu', weights_only=False)
    assert all(k.startswith('module.') for k in sd) and sd['module.bn2.num_batches_tracked'].dtype == torch_cuda.int64
    assert int(sd['module.bn2.num_batches_tracked']) == 8            # 2 epochs x 32 patches / 8
    model = engine.Model(ev.strip_module_prefix(sd), cfg)
    b = TM.make_batch(3, 32, 64, 5)
    logits, _ = model.forward(*_dev_batch(torch_cuda, b)[:3])
    assert np.isfinite(logits.cpu().numpy()).all()
    model.close()
