"""The train-mode restatement (tests/train_model.py) reproduces the reference's own training step (CPU, no GPU):
tests/golden/train_step_<cfg>.npz holds what the unmodified reference model, its compute_loss and two torch SGD steps
give in float32 (tools/make_golden_train.py); the restatement runs the same two steps in float64, its max-pools forced
to the indices the reference picked (a near-tie resolves differently in float64 and moves a whole row of a gradient).

Tolerance: the golden is float32 arithmetic on a batch of FOUR items, whose batch-norms divide by the standard deviation
of four numbers; what single precision costs there is measured, not guessed: the same restatement runs in float32 on
the same forced indices, and the gate is 4x its largest per-tensor distance (L2, relative to the tensor's norm) from the
float64 run -- the reference sums in another order than either.  A wrong formula (a missed ReLU mask, a biased variance
in the running update, an unscaled loss) is in both precisions of the restatement and O(1) away from the golden.
Biases whose gradient is zero in exact arithmetic (train_model.zero_grad_names) are compared against the norm of
their layer's weight gradient.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import train_model as TM  # noqa: E402



@pytest.mark.parametrize('name', ['p2s_max', 'p2s_max_no_feat_stn'])
def test_restatement_reproduces_the_reference_step(name):
    import torch
    from points2surf_amd import synth
    g = np.load(os.path.join(HERE, 'golden', 'train_step_%s.npz' % name))
    w, cfg = synth.make_weights(name)
    runs = {}
    for dt in (torch.float64, torch.float32):
        m = TM.TrainModel(w, cfg, dtype=dt)
        losses = []
        for step in range(2):
            forced = {p: g['pool/%d/%s' % (step, p)] for p in TM.pool_names(cfg)}
            losses.append(m.forward_backward(g['patch'], g['sub'], g['query'], g['dist_abs'], g['sign01'], g['radius'],
                                             forced=forced))
            m.step(0.01, 0.9)
        runs[dt] = (np.asarray(losses), m.grads(), m.state())
    losses, grads, state = runs[torch.float64]
    l32, g32, s32 = runs[torch.float32]
    zero = TM.zero_grad_names(grads)
    LOSS_TOL = 4 * float(np.abs(l32 / losses - 1).max())
    TOL = 4 * max([TM.rel_err(g32[k], v) for k, v in grads.items() if k not in zero] +
                  [TM.rel_err(s32[k], v) for k, v in state.items() if not k.endswith('num_batches_tracked')])
    print('float32 against float64 restatement, x4: losses %.3g, tensors %.3g' % (LOSS_TOL, TOL))
    assert LOSS_TOL < 1e-2 and TOL < 0.1
    np.testing.assert_allclose(losses, g['losses'], rtol=LOSS_TOL)
    assert sorted('state/' + k for k in state) == sorted(k for k in g.files if k.startswith('state/'))
    worst = 0.0
    errs = {}
    for k, v in state.items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == int(g['state/' + k]) == 1002
            continue
        ref, norm = g['state/' + k], float(g['state_norm/' + k])
        scale = norm * np.sqrt(ref.size / v.size)
        e = np.linalg.norm(TM.golden_view(v) - ref) / scale
        assert abs(np.linalg.norm(v) - norm) <= TOL * norm and e <= TOL, (k, e)
        if k not in grads:
            continue
        gr, gn = g['grad/' + k], float(g['grad_norm/' + k])
        if k in zero:
            wn = float(g['grad_norm/' + k[:-4] + 'weight'])
            assert np.linalg.norm(grads[k]) <= TOL * wn and gn <= TOL * wn, k
            continue
        e = np.linalg.norm(TM.golden_view(grads[k]) - gr) / (gn * np.sqrt(gr.size / grads[k].size))
        worst = max(worst, e)
        errs[k] = e
        assert abs(np.linalg.norm(grads[k]) - gn) <= TOL * gn and e <= TOL, (k, e)
    print('worst sampled gradient error', worst, sorted(errs.items(), key=lambda t: -t[1])[:3])


@pytest.mark.parametrize('name', ['p2s_max', 'p2s_max_no_feat_stn'])
def test_float32_restatement_reproduces_the_reference_losses(name):
    """in the reference's own precision the restatement is the same arithmetic: both steps' losses to float32 rounding"""
    import torch
    from points2surf_amd import synth
    g = np.load(os.path.join(HERE, 'golden', 'train_step_%s.npz' % name))
    w, cfg = synth.make_weights(name)
    m = TM.TrainModel(w, cfg, dtype=torch.float32)
    for step in range(2):
        loss = m.forward_backward(g['patch'], g['sub'], g['query'], g['dist_abs'], g['sign01'], g['radius'])
        np.testing.assert_allclose(np.asarray(loss), g['losses'][step], rtol=1e-5)
        m.step(0.01, 0.9)


def test_forced_pool_is_the_max_at_its_own_indices():
    from points2surf_amd import synth
    w, cfg = synth.make_weights('p2s_max')
    b = TM.make_batch(3, 9, 11, seed=3, pad_duplicates=True)
    a = TM.TrainModel(w, cfg)
    la = a.forward_backward(b['patch'], b['sub'], b['query'], b['dist_abs'], b['sign01'], b['radius'])
    # padded items: the lowest index wins the tie
    assert a.pools['feat_local'][0].max() <= 9 // 2 and a.pools['feat_global.stn2'][0].max() <= 11 // 2
    c = TM.TrainModel(w, cfg)
    lc = c.forward_backward(b['patch'], b['sub'], b['query'], b['dist_abs'], b['sign01'], b['radius'], forced=a.pools)
    assert la == lc
    for k, v in a.grads().items():
        assert np.array_equal(v, c.grads()[k]), k
