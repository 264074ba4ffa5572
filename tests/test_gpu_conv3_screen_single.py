"""GPU: the one-piece screen of conv3 (points2surf_amd/csrc/p2s_chain_screen.inl) equals the dense conv3 where one fp16
rounding per operand orders rows differently than fp32 does.

The screen sees t[p][c] = sum_k fp16(h_pk) fp16(w_ck), about 2^-10 relative, and the pooled value comes from the fp32 chains of
the candidates it keeps; P2S_CONV3_DENSE=1 at model creation keeps the dense conv3.  16 queries, both handles in one process on
the same inputs, compared with array_equal (0 ulp, as tests/test_gpu_conv3_screen.py): the STN pools, the features, the logits
and the SDF.

    near-duplicates      rows that differ in the 13th bit: the same or a reversed order in one fp16 piece
    tiny / large channel the margin's absolute terms and its scaling with |w_c|
    1, 33, 64, 65 points the short-tail forms"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 40938661
NQ = 16
_CACHE = {}


def _model(engine, w, cfg, dense):
    old = os.environ.get('P2S_CONV3_DENSE')
    os.environ['P2S_CONV3_DENSE'] = '1' if dense else '0'
    try:
        return engine.Model(w, cfg)
    finally:
        if old is None:
            del os.environ['P2S_CONV3_DENSE']
        else:
            os.environ['P2S_CONV3_DENSE'] = old


def _inputs(engine, fixture_cloud):
    """NQ grid queries of the fixture cloud with their kNN patches (300) and uniform sub-samples (1000); computed once, never
    written to"""
    if 'in' not in _CACHE:
        cloud = engine.Cloud(fixture_cloud)
        q = cloud.query_grid(32, 3)
        q = q[:: max(1, q.shape[0] // NQ)][:NQ].contiguous()
        _, sub = engine.Rng(SEED).subsample_uniform(cloud, NQ, 1000)
        _, patch, rad = cloud.knn_patch(q, 300, want_ids=False)
        _CACHE['in'] = (patch.contiguous(), sub.contiguous(), q, rad.contiguous())
    return _CACHE['in']


def _run(m, patch, sub, q, rad):
    import torch
    lg, sdf = m.forward(patch, sub, q, rad, want_sdf=True)
    stn = m.debug_stn_pool(patch.shape[0])
    torch.cuda.synchronize()
    cnt = m.counters()
    fl, fg = m.features(patch, sub, q)
    torch.cuda.synchronize()
    return {'logits': lg.cpu().numpy(), 'sdf': sdf.cpu().numpy(), 'feat_local': fl.cpu().numpy(), 'feat_global': fg.cpu().numpy(),
            'stn_pool': stn.cpu().numpy()}, cnt


def _both(engine, w, cfg, patch, sub, q, rad):
    out = []
    for dense in (False, True):
        m = _model(engine, w, cfg, dense)
        out.append(_run(m, patch, sub, q, rad))
        m.close()
    (scr, c_scr), (den, c_den) = out
    assert c_den['conv3_items'] == 0 and c_den['conv3_confirmed'] == 0           # the switch does switch
    return scr, c_scr, den


def _assert_equal(scr, den, what):
    for k in ('stn_pool', 'feat_local', 'feat_global', 'logits', 'sdf'):
        a, b = scr[k], den[k]
        same = np.array_equal(a, b, equal_nan=True)
        if not same:
            d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
            print('%s / %s: %d of %d values differ, largest difference %d ulp' % (what, k, int((d != 0).sum()), d.size, int(d.max())))
        assert same, (what, k)


def _report(what, c):
    items = int(c['conv3_items'])
    print('%s: conv3_items %d, conv3_items_dense %d, conv3_confirmed %d (%.2f per channel of a screened item)' % (
        what, items, int(c['conv3_items_dense']), int(c['conv3_confirmed']),
        c['conv3_confirmed'] / (1024.0 * max(1, items - int(c['conv3_items_dense'])))))


def test_near_duplicates(fixture_cloud):
    """points 100 .. 139 of one patch are point 7 times (1 + j 2^-13), j = 0 .. 39, across a tile boundary, and the same for
    points 960 .. 999 of one sub-sample: 40 rows per item whose fp16 roundings mostly coincide.  Nothing runs densely"""
    import torch
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    patch, sub = patch.clone(), sub.clone()
    f = (1.0 + torch.arange(40, device=patch.device, dtype=torch.float32) * float(2.0 ** -13)).view(40, 1)
    patch[0, 100:140] = patch[0, 7].view(1, 3) * f
    sub[2, 960:1000] = sub[2, 7].view(1, 3) * f
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('near-duplicates', c)
    _assert_equal(scr, den, 'near-duplicates')
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0


def test_tiny_and_large_channels(fixture_cloud):
    """one conv3 channel times 2^-20 (its fp16 weights are subnormal or zero) and one times 2^10, in the STN trunk and in the
    main trunk, on the default weights; the consumer's weights are divided accordingly, so the function is the same"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    w = {k: v.copy() for k, v in w.items()}
    for bn, nxt in (('feat_global.stn2.bn3', 'feat_global.stn2.fc1.weight'), ('feat_local.bn3', 'fc1_local.weight')):
        for ch, s in ((5, float(2.0 ** -20)), (9, float(2.0 ** 10))):
            w[bn + '.weight'][ch] *= s
            w[bn + '.bias'][ch] *= s
            w[nxt][:, ch] /= s
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('scaled channels', c)
    _assert_equal(scr, den, 'scaled channels')


@pytest.mark.parametrize('n', [1, 33, 64, 65])
def test_patch_sizes(n, fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    cfg_n = dict(cfg, points_per_patch=n, sub_sample_size=n)
    scr, c, den = _both(engine, w, cfg_n, patch[:, :n].contiguous(), sub[:, :n].contiguous(), q, rad)
    _report('%d points' % n, c)
    _assert_equal(scr, den, '%d points' % n)
