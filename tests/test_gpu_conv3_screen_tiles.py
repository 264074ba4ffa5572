"""GPU: the screened conv3 (points2surf_amd/csrc/p2s_chain_screen.inl) equals the dense conv3 at the tile shapes at which its
weight stream over the column tiles and its two confirm forms can go wrong.

The screen keeps one ring of weight-fragment requests running over the eight column tiles of a 64-point tile and across the
select, the queue and the confirm of each; candidates of rows >= 32 of a 16-row tail tile are confirmed by the two-chain form,
every other candidate by the plain chain, chosen per batch.  Patch and sub-sample sizes, both set to the same value:

    1          one tile, one valid row; everything else is padding
    48 / 49    a single tile with and without the 16-row tail
    64 / 65    the ring's end at a tile boundary and a one-row second tile
    112 / 113  a full tile followed by a tail and by a non-tail short tile: candidates in rows >= 32 of both kinds meet both
               confirm forms
    128        two full tiles

8 queries; screened and dense handles in one process, compared with array_equal (0 ulp, as tests/test_gpu_conv3_screen.py):
the STN pools, the features, the logits and the SDF, on the default weights and on the adversarial set p2s_max_stress (ties
and tiny channels: the queue's flush and the dense re-run).  On the default weights no item runs densely at these shapes.

The commit before this test fails it at 1 point (3239 of 16384 STN-pool values differ from the dense kernel's, none run
densely): in a tail tile with at most 32 points the dense kernel also pools rows 32 .. 47, replicas of the last point summed
by the two-chain form, which the screen had masked out as padding.  1 and 65 points keep that case covered."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 40938661
NQ = 8
SHAPES = (1, 48, 49, 64, 65, 112, 113, 128)
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
    """NQ grid queries of the fixture cloud with their 128 nearest points and 128 uniform samples; a shape takes the first n of
    each.  Computed once, never written to."""
    if 'in' not in _CACHE:
        cloud = engine.Cloud(fixture_cloud)
        q = cloud.query_grid(32, 3)
        q = q[:: max(1, q.shape[0] // NQ)][:NQ].contiguous()
        _, sub = engine.Rng(SEED).subsample_uniform(cloud, NQ, max(SHAPES))
        _, patch, rad = cloud.knn_patch(q, max(SHAPES), want_ids=False)
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


@pytest.mark.parametrize('model', ['p2s_max', 'p2s_max_stress'])
def test_tile_shapes_equal_dense(model, fixture_cloud):
    from points2surf_amd import engine, synth
    assert 'p2s_max_stress' in synth.STRESS_MODELS
    w, cfg = synth.make_weights(model)
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    for n in SHAPES:
        cfg_n = dict(cfg, points_per_patch=n, sub_sample_size=n)
        pn, sn = patch[:, :n].contiguous(), sub[:, :n].contiguous()
        out = []
        for dense in (False, True):
            m = _model(engine, w, cfg_n, dense)
            out.append(_run(m, pn, sn, q, rad))
            m.close()
        (scr, c), (den, c_den) = out
        print('%s, %d points: conv3_items %d, conv3_items_dense %d, conv3_confirmed %d' % (
            model, n, int(c['conv3_items']), int(c['conv3_items_dense']), int(c['conv3_confirmed'])))
        assert c_den['conv3_items'] == 0 and c_den['conv3_confirmed'] == 0       # the switch does switch
        assert c['conv3_items'] == 4 * NQ                                       # STN and main pass of both encoders
        if model == 'p2s_max':
            assert c['conv3_items_dense'] == 0, n
        for k in ('stn_pool', 'feat_local', 'feat_global', 'logits', 'sdf'):
            a, b = scr[k], den[k]
            same = np.array_equal(a, b, equal_nan=True)
            if not same:
                d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
                print('%s, %d points / %s: %d of %d values differ, largest difference %d ulp' % (
                    model, n, k, int((d != 0).sum()), d.size, int(d.max())))
            assert same, (model, n, k)
