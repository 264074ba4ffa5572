"""GPU: the pool bound in the select of the screened conv3 (points2surf_amd/csrc/p2s_chain_screen.inl) -- from an item's second
tile on, a product is a candidate iff t >= max(R - mu, E - mu / 2), E the exact fp32 maximum of the rows confirmed so far --
leaves the screened path bit-identical to the dense conv3 (P2S_CONV3_DENSE=1), and confirms fewer chains.

16 queries of the fixture cloud at grid 32, both handles in one process on the same inputs, array_equal on the STN pools, the
features, the logits and the SDF (the pattern of tests/test_gpu_conv3_screen_single.py, whose helpers are used):

    winner early     rows of later tiles a hair BELOW a row of tile 0: inside the half margin of a confirmed E
    winner late      the same rows a hair ABOVE it: records are broken after E is set
    duplicates       a point of tile 0 again in the last full tile: t == R and fl == E across tiles
    65, 80, 128, 129 a full tile and a tail of 1 / 16 (row 32 stands for the replicas of the short tail, E set by the tile
                     before), two full tiles, two full tiles and a tail of 1
    scaled channels  one conv3 channel x 2^-20, one x 2^10 in all four trunks on the winner-early inputs: the absolute terms
                     of mu / 2
    counters         nothing runs densely and the confirmed chains per channel fall to 0.85 of the parent commit's at most

NaN inputs and patches of identical points are in tests/test_gpu_conv3_screen.py."""
import pytest

from test_gpu_conv3_screen_single import NQ, _assert_equal, _both, _inputs, _report

pytestmark = pytest.mark.gpu

# conv3_confirmed / (1024 * conv3_items) of the parent commit (f29a457: the R rule alone) on the 16 queries of _inputs with the
# default weights, measured through the parent's own tree and library on the MI355X that measured this commit: 529921 chains
# over 64 items
PARENT_CONFIRMED_PER_CHANNEL = 529921 / (1024.0 * 64)


def _near_copies(engine, fixture_cloud, sign):
    """points 200 .. 239 of patch 0 and 900 .. 939 of sub-sample 2 are point 7 (tile 0) times (1 + sign j 2^-13), j = 0 .. 39"""
    import torch
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    patch, sub = patch.clone(), sub.clone()
    f = (1.0 + sign * torch.arange(40, device=patch.device, dtype=torch.float32) * float(2.0 ** -13)).view(40, 1)
    patch[0, 200:240] = patch[0, 7].view(1, 3) * f
    sub[2, 900:940] = sub[2, 7].view(1, 3) * f
    return patch, sub, q, rad


@pytest.mark.parametrize('sign,what', [(-1.0, 'winner early'), (1.0, 'winner late')])
def test_near_ties_across_tiles(sign, what, fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _near_copies(engine, fixture_cloud, sign)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report(what, c)
    _assert_equal(scr, den, what)
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0


def test_duplicate_in_tile_0_and_in_the_last_full_tile(fixture_cloud):
    """every patch holds its point 7 again as point 200 (tile 3 of 300 points), every sub-sample as point 900 (tile 14 of 1000)"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    patch, sub = patch.clone(), sub.clone()
    patch[:, 200] = patch[:, 7]
    sub[:, 900] = sub[:, 7]
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('duplicates', c)
    _assert_equal(scr, den, 'duplicates')
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0


@pytest.mark.parametrize('n', [65, 80, 128, 129])
def test_patch_sizes(n, fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    cfg_n = dict(cfg, points_per_patch=n, sub_sample_size=n)
    scr, c, den = _both(engine, w, cfg_n, patch[:, :n].contiguous(), sub[:, :n].contiguous(), q, rad)
    _report('%d points' % n, c)
    _assert_equal(scr, den, '%d points' % n)
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0


def test_tiny_and_large_channels_on_the_winner_early_inputs(fixture_cloud):
    """one conv3 channel times 2^-20 and one times 2^10 in the STN trunk and the main trunk of both encoders, the consumer's
    weights divided accordingly, so the function is the same"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    w = {k: v.copy() for k, v in w.items()}
    for bn, nxt in (('feat_global.stn2.bn3', 'feat_global.stn2.fc1.weight'), ('feat_local.stn2.bn3', 'feat_local.stn2.fc1.weight'),
                    ('feat_global.bn3', 'fc1_global.weight'), ('feat_local.bn3', 'fc1_local.weight')):
        for ch, s in ((5, float(2.0 ** -20)), (9, float(2.0 ** 10))):
            w[bn + '.weight'][ch] *= s
            w[bn + '.bias'][ch] *= s
            w[nxt][:, ch] /= s
    patch, sub, q, rad = _near_copies(engine, fixture_cloud, -1.0)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('scaled channels', c)
    _assert_equal(scr, den, 'scaled channels')
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0


def test_fewer_chains_are_confirmed_and_nothing_runs_densely(fixture_cloud):
    """the default weights on the 16 queries: 0.85 of the parent's confirmed chains per channel at most (the CPU model of
    tests/test_conv3_screen_pool_bound_cpu.py says 0.72 on its 8 queries; the device kept 8.09 where that model said 10.2)"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('default weights', c)
    _assert_equal(scr, den, 'default weights')
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0
    per_channel = c['conv3_confirmed'] / (1024.0 * c['conv3_items'])
    print('confirmed per channel: %.4f, parent %.4f, ratio %.4f' % (per_channel, PARENT_CONFIRMED_PER_CHANNEL,
                                                                   per_channel / PARENT_CONFIRMED_PER_CHANNEL))
    assert per_channel <= 0.85 * PARENT_CONFIRMED_PER_CHANNEL
