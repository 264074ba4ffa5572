"""GPU: the screened conv3 of the fp32 encoders (points2surf_amd/csrc/p2s_chain_screen.inl) returns what the dense conv3
returns.

The fp32 chain kernel screens the 128 -> 1024 layer on fp16-pair MFMAs and computes in fp32 only the products that can be
the maximum over the item's points; P2S_CONV3_DENSE=1 at model creation keeps the dense conv3 (the A/B switch).  Every test
builds both handles in one process on the same inputs -- 8 .. 64 queries, patches of 300 and sub-samples of 1000 points
(both 16-row tail-tile shapes) -- and compares bit for bit.

Equality bound: the fmaf chain of the confirm step reproduces the fp32 MFMA chain bit for bit on gfx950 (measured with these
tests: every compared value identical), so the recorded bound is 0 ulp and the comparison is array_equal.

What is compared: the pooled 1024-vectors of the STN pass of both encoders (read from the model's workspace through the
test hook Model.debug_stn_pool) and of the main pass (Model.features), the logits and the SDF.

An item the screen cannot decide runs again through the dense conv3 inside the same kernel (no side buffer, no per-call
limit): counters()['conv3_items_dense'] counts them."""
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


def _inputs(engine, fixture_cloud, nq=NQ):
    """nq grid queries of the fixture cloud with their kNN patches (300) and uniform sub-samples (1000); computed once"""
    if nq not in _CACHE:
        cloud = engine.Cloud(fixture_cloud)
        q = cloud.query_grid(32, 3)
        q = q[:: max(1, q.shape[0] // nq)][:nq].contiguous()
        _, sub = engine.Rng(SEED).subsample_uniform(cloud, nq, 1000)
        _, patch, rad = cloud.knn_patch(q, 300, want_ids=False)
        _CACHE[nq] = (patch.contiguous(), sub.contiguous(), q, rad.contiguous())
    return _CACHE[nq]


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


@pytest.mark.parametrize('model', ['p2s_max', 'p2s_max_stress', 'p2s_vanilla_stress'])
def test_screened_equals_dense(model, fixture_cloud):
    from points2surf_amd import engine, synth
    assert set(synth.STRESS_MODELS) == {'p2s_max_stress', 'p2s_vanilla_stress'}
    w, cfg = synth.make_weights(model)
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report(model, c)
    assert c['conv3_items'] == 4 * NQ                      # STN and main pass of both encoders
    _assert_equal(scr, den, model)


def test_cap_on_confirmed_products(fixture_cloud):
    """a kernel that confirmed everything would pass equality and be slow: on the default weights nothing runs densely and at
    most 16 fp32 chains per pooled channel are run (a condition, not a measurement: a random order gives 1 + ln(tiles), 3 - 4)"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    m = _model(engine, w, cfg, False)
    _, c = _run(m, patch, sub, q, rad)
    m.close()
    _report('p2s_max, default weights', c)
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0
    assert c['conv3_confirmed'] / (c['conv3_items'] * 1024.0) <= 16.0


def test_ties_and_replicated_rows(fixture_cloud):
    """exact duplicates tie in every channel; the last tile of every item is padded with replicas of its last point (300 = 4 x
    64 + 44, 1000 = 15 x 64 + 40); a patch of identical points ties everywhere and must take the dense route"""
    import torch
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    patch, sub = patch.clone(), sub.clone()
    patch[0, 100:140] = patch[0, 7]                        # 40 exact duplicates of one point, across a tile boundary
    patch[1, 260:300] = patch[1, 259]                      # the whole last tile of the patch = one point, then its replicas
    sub[2, 960:1000] = sub[2, 3]                           # the same for the 1000-point item
    patch[3, :] = patch[3, 0]                              # 300 identical points
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('ties', c)
    _assert_equal(scr, den, 'ties')
    assert c['conv3_items_dense'] >= 2                     # the identical patch: its STN and its main pass
    # alone, so that the count is exact
    one = [t[3:4].contiguous() for t in (patch, sub, q, rad)]
    m = _model(engine, w, cfg, False)
    _, c1 = _run(m, *one)
    m.close()
    assert c1['conv3_items'] == 4 and c1['conv3_items_dense'] == 2


def _scaled_conv3(w, c, s, trunk):
    """the same function: conv3's output channel c of a trunk times s (bn3 is affine and follows conv3 directly), the consumer's
    weights for that channel divided by s (max-pool and ReLU are positively homogeneous, powers of two are exact)"""
    w2 = {k: v.copy() for k, v in w.items()}
    if trunk == 'stn':
        bn, nxt = 'feat_global.stn2.bn3', 'feat_global.stn2.fc1.weight'
    else:
        bn, nxt = 'feat_local.bn3', 'fc1_local.weight'
    w2[bn + '.weight'][c] *= s
    w2[bn + '.bias'][c] *= s
    w2[nxt][:, c] /= s
    return w2


def test_margin_is_honest_for_tiny_and_large_channels(fixture_cloud):
    """one conv3 channel times 2^-20 (its fp16 weight pieces fall below the normal range: the margin's absolute terms must
    cover them) and one times 2^10, in the STN trunk and in the main trunk: equal to dense, no error.  Nothing leaves the half
    range here -- the screen reads the conv2 output, which these scalings do not touch, and the weights stay far inside it
    (2^10 x 0.2) -- and the tiny channel's margin, 2^-13 (|w_c| + 2^-10) H with |w_c| ~ 2^-20, is about a tenth of the spread
    of its values (~ |w_c| H): a few candidates per tile in one column, far from the queue's 256.  So no item runs densely;
    the items that do leave the range are those of test_activations_beyond_the_half_range_run_densely"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    for trunk in ('stn', 'main'):
        w = _scaled_conv3(_scaled_conv3(w, 5, float(2.0 ** -20), trunk), 9, float(2.0 ** 10), trunk)
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('scaled channels', c)
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0
    _assert_equal(scr, den, 'scaled channels')


def test_activations_beyond_the_half_range_run_densely(fixture_cloud):
    """every item leaves the half range where the screen reads it -- the conv2 output: eight bn2 channels of every trunk times
    2^24, conv3's input columns divided by it (the 'chain' construction of test_gpu_fp16_fallback.py) -- with 64 queries in one
    call: every item is re-run densely inside the kernel -- there is no side buffer to overflow -- and the results are the
    dense kernel's"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    w2 = {k: v.copy() for k, v in w.items()}
    s = float(2 ** 24)
    for trunk in ('feat_local', 'feat_global', 'feat_local.stn2', 'feat_global.stn2'):
        for c in range(8):
            w2[trunk + '.bn2.weight'][c] *= s
            w2[trunk + '.bn2.bias'][c] *= s
            w2[trunk + '.conv3.weight'][:, c, :] /= s
    patch, sub, q, rad = _inputs(engine, fixture_cloud, 64)
    scr, c, den = _both(engine, w2, cfg, patch, sub, q, rad)
    _report('beyond the half range', c)
    assert c['conv3_items'] == 4 * 64 and c['conv3_items_dense'] == c['conv3_items']
    _assert_equal(scr, den, 'beyond the half range')


def test_non_finite_input_poisons_like_dense(fixture_cloud):
    """one NaN coordinate in one query of a batch of 8: the outputs of all 8 are the dense kernel's"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = [t[:8].clone() for t in _inputs(engine, fixture_cloud)]
    patch[5, 17, 1] = float('nan')
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    assert np.isnan(den['logits'][5]).all() and not np.isnan(den['logits'][[0, 1, 2, 3, 4, 6, 7]]).any()
    _assert_equal(scr, den, 'non-finite input')
