"""GPU: the main encoder pass that starts at conv1 from the stem the STN pass saved (p2s_chain_reuse_kernel)
equals the pass that recomputes the stem, bit for bit.

The STN pass of an fp32 model with a screened conv3 and a max pool writes conv0b's output of every 64-point tile to the
workspace in the order conv1 reads its A operand (16 KB per tile); the main pass loads it and has no point, centre, rotation,
conv0a or conv0b.  Only where conv1's input comes from changes, so three handles in one process -- default, stem_reuse=False
(a member of the model configuration: the library's environment switches are capped at 20, tests/test_abi.py) and
P2S_CONV3_DENSE=1 -- must agree in the STN pools, both features, the logits and the SDF with array_equal (0 ulp).

Sizes (patch, sub-sample), 8 queries of the fixture cloud:
    (1, 1)        one valid row
    (48, 49)      a tail and a non-tail single tile, and (64, 65), (113, 128): different tile counts in the two branches, whose
    (64, 65)      regions of the workspace lie behind each other: a wrong offset or stride reads another item's tiles
    (113, 128)
    (300, 1000)   the real sizes, once: 5 + 16 tiles per query
p2s_max_stress (ties and tiny channels) sends items through the dense re-run inside the kernel, which reads the stem a second
time; p2s_vanilla has a rotation and a QSTN launch in front of the passes.  Beside the values: the counter stem_items_reused,
a second call with fewer queries on the same handle (stale tiles), non-finite coordinates (the saved stem hides a NaN behind
fmaxf: the verdict travels in a flag), the modes that must not reuse, and the cap of the region."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 40938661
NQ = 8
EXTRA = 3                      # other queries, for the second call on the same handle
SIZES = ((1, 1), (48, 49), (64, 65), (113, 128), (300, 1000))
KEYS = ('stn_pool', 'feat_local', 'feat_global', 'logits', 'sdf')
_CACHE = {}


def _model(engine, w, cfg, dense=False, **stem):
    """a handle with the given stem settings (stem_reuse, stem_reuse_max_mb: configuration) and conv3 (P2S_CONV3_DENSE: read at
    creation)"""
    old = os.environ.get('P2S_CONV3_DENSE')
    os.environ['P2S_CONV3_DENSE'] = '1' if dense else '0'
    try:
        return engine.Model(w, dict(cfg, **stem))
    finally:
        if old is None:
            del os.environ['P2S_CONV3_DENSE']
        else:
            os.environ['P2S_CONV3_DENSE'] = old


def _inputs(engine, fixture_cloud):
    """NQ + EXTRA grid queries of the fixture cloud with their 300 nearest points and 1000 uniform samples; a size takes the first
    points of each.  Computed once, never written to."""
    if 'in' not in _CACHE:
        n = NQ + EXTRA
        cloud = engine.Cloud(fixture_cloud)
        q = cloud.query_grid(32, 3)
        q = q[:: max(1, q.shape[0] // n)][:n].contiguous()
        _, sub = engine.Rng(SEED).subsample_uniform(cloud, n, 1000)
        _, patch, rad = cloud.knn_patch(q, 300, want_ids=False)
        _CACHE['in'] = (patch.contiguous(), sub.contiguous(), q, rad.contiguous())
    return _CACHE['in']


def _sized(inputs, k, n, rows=slice(0, NQ)):
    patch, sub, q, rad = inputs
    return patch[rows, :k].contiguous(), sub[rows, :n].contiguous(), q[rows].contiguous(), rad[rows].contiguous()


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


def _assert_equal(a, b, what, rows=None):
    for k in KEYS:
        x, y = a[k], b[k]
        if rows is not None:
            if k == 'stn_pool':                 # [2][queries][1024]
                x, y = x.reshape(2, -1, 1024)[:, rows], y.reshape(2, -1, 1024)[:, rows]
            else:
                x, y = x[rows], y[rows]
        same = np.array_equal(x, y, equal_nan=True)
        if not same:
            bad = ~((x == y) | (np.isnan(x) & np.isnan(y)))
            print('%s / %s: %d of %d values differ' % (what, k, int(bad.sum()), bad.size))
        assert same, (what, k)


def _three_handles(engine, w, cfg, inputs, k, n, what):
    """default, reuse off, dense conv3 at one size: equal outputs, and the counters of each"""
    cfg_n = dict(cfg, points_per_patch=k, sub_sample_size=n)
    args = _sized(inputs, k, n)
    res = []
    for env in ({}, {'stem_reuse': False}, {'dense': True}):
        m = _model(engine, w, cfg_n, **env)
        res.append(_run(m, *args))
        m.close()
    (reuse, c), (off, c_off), (dense, c_dense) = res
    print('%s: stem_items_reused %d, conv3_items %d, conv3_items_dense %d, conv3_confirmed %d' % (
        what, int(c['stem_items_reused']), int(c['conv3_items']), int(c['conv3_items_dense']), int(c['conv3_confirmed'])))
    assert c['stem_items_reused'] == 2 * NQ                   # both encoders of every query, per forward
    assert c_off['stem_items_reused'] == 0 and c_dense['stem_items_reused'] == 0
    assert c['conv3_items'] == 4 * NQ and c_off['conv3_items'] == 4 * NQ and c_dense['conv3_items'] == 0
    # the screen saw the same activations: the same candidates, the same items it could not decide
    assert c['conv3_confirmed'] == c_off['conv3_confirmed'] and c['conv3_items_dense'] == c_off['conv3_items_dense']
    _assert_equal(reuse, off, what + ', reuse against recompute')
    _assert_equal(reuse, dense, what + ', reuse against the dense conv3')
    return c


@pytest.mark.parametrize('model', ['p2s_max', 'p2s_max_stress'])
def test_reuse_equals_recompute(model, fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights(model)
    inputs = _inputs(engine, fixture_cloud)
    dense_items = 0
    for k, n in SIZES:
        c = _three_handles(engine, w, cfg, inputs, k, n, '%s (%d, %d)' % (model, k, n))
        dense_items += int(c['conv3_items_dense'])
    if model == 'p2s_max_stress':
        # items the screen hands to the dense conv3 read the stem twice (the recomputing build shows them at these sizes too:
        # the counts are asserted equal above)
        assert dense_items > 0


def test_reuse_equals_recompute_with_qstn(fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_vanilla')
    _three_handles(engine, w, cfg, _inputs(engine, fixture_cloud), 49, 113, 'p2s_vanilla (49, 113)')


def test_second_call_with_fewer_queries_reads_no_stale_tile(fixture_cloud):
    """8 queries, then 3 others on the same handle: the regions of the two branches move with the number of queries of the call"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    inputs = _inputs(engine, fixture_cloud)
    k, n = 113, 128
    cfg_n = dict(cfg, points_per_patch=k, sub_sample_size=n)
    others = _sized(inputs, k, n, slice(NQ, NQ + EXTRA))
    m = _model(engine, w, cfg_n)
    _run(m, *_sized(inputs, k, n))
    second, c = _run(m, *others)
    m.close()
    fresh = _model(engine, w, cfg_n)
    want, _ = _run(fresh, *others)
    fresh.close()
    assert c['stem_items_reused'] == 2 * EXTRA
    _assert_equal(second, want, 'second call')


def test_non_finite_coordinates_poison_as_without_reuse(fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    inputs = _inputs(engine, fixture_cloud)
    k, n = 113, 128
    cfg_n = dict(cfg, points_per_patch=k, sub_sample_size=n)
    patch, sub, q, rad = _sized(inputs, k, n)
    clean_args = (patch, sub, q, rad)
    patch_bad, sub_bad = patch.clone(), sub.clone()
    patch_bad[2, 100, 1] = float('nan')          # second tile of the patch of query 2
    sub_bad[5, 70, 0] = float('inf')             # second tile of the sub-sample of query 5
    out = {}
    for name, env in (('reuse', {}), ('off', {'stem_reuse': False})):
        m = _model(engine, w, cfg_n, **env)
        out[name + '_clean'], _ = _run(m, *clean_args)
        out[name], c = _run(m, patch_bad, sub_bad, q, rad)
        m.close()
        assert c['stem_items_reused'] == (2 * NQ if name == 'reuse' else 0)
    _assert_equal(out['reuse'], out['off'], 'non-finite inputs')
    # the pooled features of the two poisoned items are NaN in every channel (the kernel's verdict, from the flag)
    assert np.isnan(out['reuse']['feat_local'][2]).all() and np.isnan(out['reuse']['feat_global'][5]).all()
    others = [i for i in range(NQ) if i not in (2, 5)]
    _assert_equal(out['reuse'], out['reuse_clean'], 'the other six queries', rows=others)
    assert np.isfinite(out['reuse']['sdf'][others]).all()


@pytest.mark.parametrize('mode', ['sum', 'fp16_pair'])
def test_modes_that_do_not_reuse(mode, fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max_sum' if mode == 'sum' else 'p2s_max')
    if mode == 'fp16_pair':
        cfg = dict(cfg, encoder_bf16=4)
    inputs = _inputs(engine, fixture_cloud)
    k, n = 113, 128
    cfg_n = dict(cfg, points_per_patch=k, sub_sample_size=n)
    res = []
    for env in ({}, {'stem_reuse': False}):
        m = _model(engine, w, cfg_n, **env)
        res.append(_run(m, *_sized(inputs, k, n)))
        m.close()
    (a, c), (b, c_off) = res
    assert c['stem_items_reused'] == 0 and c_off['stem_items_reused'] == 0
    _assert_equal(a, b, mode)


def test_region_beyond_the_cap_is_not_reserved(fixture_cloud):
    """8 queries of 5 + 16 tiles are 2.6 MB of stem: with a cap of 1 MB the chunk is reserved without the region and recomputes"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    inputs = _inputs(engine, fixture_cloud)
    k, n = 300, 1000
    res = []
    for env in ({'stem_reuse_max_mb': 1}, {'stem_reuse': False}):
        m = _model(engine, w, cfg, **env)
        res.append(_run(m, *_sized(inputs, k, n)))
        m.close()
    (a, c), (b, _) = res
    assert c['stem_items_reused'] == 0
    _assert_equal(a, b, 'capped')
