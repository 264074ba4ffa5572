"""GPU: the candidate mask of the screened conv3 built through the carry (points2surf_amd/csrc/p2s_chain_screen.inl, r13) --
rows 31 .. 0 of a lane's column are compared into a carry register and shifted into the mask by add-with-carry, so that row j
ends at bit j -- leaves the screened path bit-identical to the dense conv3 (P2S_CONV3_DENSE=1).

Both handles in one process on the same inputs, array_equal (0 ulp) on the STN pools (the STN pass of both branches), the two
features (the main pass of both branches), the logits and the SDF:

    small shapes   1, 31, 32, 33, 48, 49, 63, 64, 65 and 129 points per item, 2 queries of the fixture cloud: the short tail with
                   the row-32 replica up to its last size (32), the 16-row tail from its first size (33) to its last (48), the
                   single full tile from 49 on, a tile boundary followed by a tail of 1 -- every form of vmask and of the tail --
                   with the default weights and with the adversarial p2s_max_stress, with the main pass reusing the STN pass's
                   stem (p2s_chain_save_kernel / p2s_chain_reuse_kernel) and recomputing it (p2s_chain_kernel<false, true>).
                   The dense reference of a (weights, size) pair is computed once and shared
    row coverage   one 64-point tile per branch whose every row 0 .. 63 is the clear pooled argmax of at least one channel in
                   each of the four pools (asserted first on the CPU with oracle/torch_port.py on the same inputs, so the case
                   cannot pass vacuously): a bit of the mask that stands for another row than the queue decodes loses that
                   row's winners, and the pooled value with them"""
import numpy as np
import pytest

from test_gpu_conv3_screen_single import _assert_equal, _inputs, _report, _run
from test_gpu_stem_reuse import _model

pytestmark = pytest.mark.gpu

NQ = 2
SIZES = (1, 31, 32, 33, 48, 49, 63, 64, 65, 129)
MODELS = ('p2s_max', 'p2s_max_stress')
COVER_SEED = 10            # chosen on the CPU: test_every_row_of_a_tile_wins_a_channel asserts what it was chosen for
_DENSE = {}


def _dense(engine, key, w, cfg, args):
    """the dense conv3's outputs on `args`, once per key; never written to"""
    if key not in _DENSE:
        m = _model(engine, w, cfg, dense=True)
        _DENSE[key], c = _run(m, *args)
        m.close()
        assert c['conv3_items'] == 0 and c['conv3_confirmed'] == 0           # the switch does switch
    return _DENSE[key]


def _screened(engine, w, cfg, args, stem_reuse):
    m = _model(engine, w, cfg, stem_reuse=stem_reuse)
    out, c = _run(m, *args)
    m.close()
    n = args[0].shape[0]
    assert c['conv3_items'] == 4 * n
    assert c['stem_items_reused'] == (2 * n if stem_reuse else 0)           # the kernels meant are the kernels that ran
    return out, c


@pytest.mark.parametrize('stem_reuse', [True, False], ids=['reuse', 'recompute'])
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('model', MODELS)
def test_small_shapes(model, n, stem_reuse, fixture_cloud):
    import points2surf_amd.synth as synth
    from points2surf_amd import engine
    assert model == 'p2s_max' or model in synth.STRESS_MODELS
    w, cfg = synth.make_weights(model)
    cfg = dict(cfg, points_per_patch=n, sub_sample_size=n)
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    args = (patch[:NQ, :n].contiguous(), sub[:NQ, :n].contiguous(), q[:NQ].contiguous(), rad[:NQ].contiguous())
    what = '%s, %d points, %s' % (model, n, 'reuse' if stem_reuse else 'recompute')
    den = _dense(engine, (model, n), w, cfg, args)
    scr, c = _screened(engine, w, cfg, args, stem_reuse)
    _report(what, c)
    _assert_equal(scr, den, what)
    if model == 'p2s_max':
        assert c['conv3_items_dense'] == 0


def _cover_inputs():
    """64 directions per branch: points on a sphere are all extreme, so every one of them wins channels"""
    rng = np.random.default_rng(COVER_SEED)
    d = rng.standard_normal((2, 64, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    patch, sub = d[:1].astype(np.float32), (0.5 * d[1:]).astype(np.float32)
    q = rng.uniform(-0.1, 0.1, (1, 3)).astype(np.float32)
    return patch, sub, q, np.full((1,), 0.1, np.float32)


def _pre_pool(tp, x, pre):
    """what the two conv3 of encoder `pre` hand to their max pools, [rows, 1024] each: the STN trunk's and the main trunk's
    (the layers of TorchPort._feat and ._trunk, stopped before the max)"""
    import torch
    x = tp._conv_bn(x, pre + '.conv0a', pre + '.bn0a')
    x = tp._conv_bn(x, pre + '.conv0b', pre + '.bn0b')
    s = tp._conv_bn(x, pre + '.stn2.conv1', pre + '.stn2.bn1')
    s = tp._conv_bn(s, pre + '.stn2.conv2', pre + '.stn2.bn2')
    s = tp._conv_bn(s, pre + '.stn2.conv3', pre + '.stn2.bn3')
    t = (tp._trunk(x, pre + '.stn2') + torch.eye(64).view(1, 4096)).view(-1, 64, 64)
    y = tp._conv_bn(torch.bmm(t, x), pre + '.conv1', pre + '.bn1')
    y = tp._conv_bn(y, pre + '.conv2', pre + '.bn2')
    y = tp._conv_bn(y, pre + '.conv3', pre + '.bn3', relu=False)
    return s[0].T.numpy(), y[0].T.numpy()


def _clear_winners(a):
    """rows that hold a channel's maximum by more than 1e-4 of it: a hundred times what two fp32 evaluations of the chain differ by"""
    srt = np.sort(a, axis=0)
    top, second = srt[-1], srt[-2]
    clear = top - second > 1e-4 * np.maximum(np.abs(top), np.abs(second))
    return set(a.argmax(0)[clear].tolist())


def test_every_row_of_a_tile_wins_a_channel():
    import torch
    from oracle.torch_port import TorchPort
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    cfg = dict(cfg, points_per_patch=64, sub_sample_size=64)
    patch, sub, q, rad = _cover_inputs()
    # first, on the CPU: every row 0 .. 63 is the argmax of some channel, in the STN pass and in the main pass of both branches
    tp = TorchPort(w, cfg)
    with torch.no_grad():
        P = torch.from_numpy(patch).transpose(1, 2).contiguous()
        S = (torch.from_numpy(sub) - torch.from_numpy(q).unsqueeze(1)).transpose(1, 2).contiguous()
        pools = dict(zip(('local STN', 'local main'), _pre_pool(tp, P, 'feat_local')))
        pools.update(zip(('global STN', 'global main'), _pre_pool(tp, S, 'feat_global')))
    for name, a in pools.items():
        rows = _clear_winners(a)
        print('%s pass: %d of 64 rows win a channel' % (name, len(rows)))
        assert rows == set(range(64)), (name, sorted(set(range(64)) - rows))
    # then the kernels
    args = tuple(torch.from_numpy(t).cuda() for t in (patch, sub, q, rad))
    den = _dense(engine, 'cover', w, cfg, args)
    for name, a in (('local main', den['feat_local']), ('global main', den['feat_global'])):
        print('%s pool, dense kernel against the CPU: max |difference| %.3g' % (name, float(np.abs(a[0] - pools[name].max(0)).max())))
    for stem_reuse in (True, False):
        what = 'row coverage, %s' % ('reuse' if stem_reuse else 'recompute')
        scr, c = _screened(engine, w, cfg, args, stem_reuse)
        _report(what, c)
        _assert_equal(scr, den, what)
        assert c['conv3_items_dense'] == 0
