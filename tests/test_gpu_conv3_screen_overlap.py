"""GPU: the two-deep column-tile pipeline of the screened conv3 (points2surf_amd/csrc/p2s_chain_screen.inl, r11) -- the MFMAs of
column tile ct + 1 are issued into a second accumulator set while column tile ct is selected -- leaves the screened path
bit-identical to the dense conv3 (P2S_CONV3_DENSE=1) and its candidate set where it was.

16 queries of the fixture cloud at grid 32, both handles in one process on the same inputs, array_equal on the STN pools, the
features, the logits and the SDF (the helpers of tests/test_gpu_conv3_screen_single.py):

    point counts     1, 33, 64, 65, 128, 129 points per item: a lone short tail with the row-32 replica, a tail with rows >= 32,
                     one and two full tiles, a tile boundary followed by a tail of 1 -- the pipeline's prologue and its last
                     stage at every tile shape -- and the default 300 / 1000
    edge column tiles near-ties in the first and the last column tile of a wave (the pipeline's prologue and its drain): conv3
                     channels 0, 31, 224, 255, 256 and 1023 of all four trunks times 2^-20, where the margin's absolute terms
                     dominate and several rows lie within it, on the winner-early and the winner-late inputs
    fall-back paths  a patch of identical points (the queue overflows with MFMAs of the next column tile issued), one NaN
                     coordinate, one item whose conv2 output leaves the half range: conv3_items_dense counts the two passes of
                     the first and of the last and the main pass of the second, and nothing else
    candidate set    conv3_confirmed on the default weights equals the parent commit's count"""
import numpy as np
import pytest

from test_gpu_conv3_screen_single import NQ, _assert_equal, _both, _inputs, _model, _report, _run
from test_gpu_conv3_screen_pool_bound import _near_copies

pytestmark = pytest.mark.gpu

# conv3_confirmed of the parent commit (675f37c: one accumulator set, the select behind its column tile's MFMAs) on the 16
# queries of _inputs with the default weights, measured through the parent's own tree and library on an MI355X: 64 items,
# none of them dense.  The candidate set is a function of the item alone, so the count is exact
PARENT_CONFIRMED = 399114

EDGE_CHANNELS = (0, 31, 224, 255, 256, 1023)
TRUNKS = (('feat_global.stn2.bn3', 'feat_global.stn2.fc1.weight'), ('feat_local.stn2.bn3', 'feat_local.stn2.fc1.weight'),
          ('feat_global.bn3', 'fc1_global.weight'), ('feat_local.bn3', 'fc1_local.weight'))


@pytest.mark.parametrize('n', [1, 33, 64, 65, 128, 129, None])
def test_point_counts(n, fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    if n is not None:
        cfg = dict(cfg, points_per_patch=n, sub_sample_size=n)
        patch, sub = patch[:, :n].contiguous(), sub[:, :n].contiguous()
    what = '%s points' % (n if n is not None else '300 / 1000')
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report(what, c)
    _assert_equal(scr, den, what)
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0


@pytest.mark.parametrize('sign,what', [(-1.0, 'winner early'), (1.0, 'winner late')])
def test_near_ties_in_the_edge_column_tiles(sign, what, fixture_cloud):
    """the first and the last lane of the first and the last column tile of wave 0, the first column tile of wave 1 and the
    last channel of all; the consumer's weights are divided accordingly, so the function is the same"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    w = {k: v.copy() for k, v in w.items()}
    s = float(2.0 ** -20)
    for bn, nxt in TRUNKS:
        for ch in EDGE_CHANNELS:
            w[bn + '.weight'][ch] *= s
            w[bn + '.bias'][ch] *= s
            w[nxt][:, ch] /= s
    patch, sub, q, rad = _near_copies(engine, fixture_cloud, sign)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('edge column tiles, ' + what, c)
    _assert_equal(scr, den, 'edge column tiles, ' + what)
    # no claim on conv3_items_dense: with two such channels in a column tile and forty near-copies in a tile a queue may
    # overflow in the middle of the column-tile loop (one item of the winner-early inputs does), which is a path to cover
    assert c['conv3_items'] == 4 * NQ


def test_fall_back_paths_count_their_items_and_no_others(fixture_cloud):
    """query 3: 300 identical points, every product of a column tile ties and the queue overflows: its STN pass and its main
    pass run densely.  Query 5: one NaN coordinate.  That is no reason to run densely -- the ReLU of the first layer is an
    fmaxf, which drops the NaN, and the item is poisoned at the end as in the dense kernel -- so its STN pass stays screened;
    but the poisoned STN output is the feature transform of its main pass, whose folded conv1 weights are then NaN and whose
    conv1 output is fmaxf(NaN, 0) = 0 in every row: 300 identical rows, which overflow the queue like query 3, one dense item.
    Query 7: one sub-sample point far outside, so that the conv2 output is finite and beyond the half range in the STN pass
    and in the main pass of the encoder that reads the sub-sample.  Five dense items, and no others"""
    import torch
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    patch, sub = patch.clone(), sub.clone()
    patch[3, :] = patch[3, 0]
    patch[5, 17, 1] = float('nan')
    sub[7, 11] = torch.tensor([3.0e5, -2.0e5, 1.0e5], device=sub.device)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('fall-back paths', c)
    _assert_equal(scr, den, 'fall-back paths')
    assert np.isnan(den['logits'][5]).all()
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 5
    # which items: each special query alone, and the thirteen others together
    m = _model(engine, w, cfg, False)
    dense = {}
    for i in (3, 5, 7):
        _, ci = _run(m, *[t[i:i + 1].contiguous() for t in (patch, sub, q, rad)])
        assert ci['conv3_items'] == 4
        dense[i] = int(ci['conv3_items_dense'])
    rest = [i for i in range(NQ) if i not in (3, 5, 7)]
    _, cr = _run(m, *[t[rest].contiguous() for t in (patch, sub, q, rad)])
    m.close()
    print('dense items of queries 3, 5, 7 alone:', dense, '; of the others:', int(cr['conv3_items_dense']))
    assert dense == {3: 2, 5: 1, 7: 2}
    assert cr['conv3_items'] == 4 * len(rest) and cr['conv3_items_dense'] == 0


def test_the_candidate_set_did_not_move(fixture_cloud):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max')
    patch, sub, q, rad = _inputs(engine, fixture_cloud)
    scr, c, den = _both(engine, w, cfg, patch, sub, q, rad)
    _report('default weights', c)
    _assert_equal(scr, den, 'default weights')
    assert c['conv3_items'] == 4 * NQ and c['conv3_items_dense'] == 0
    print('conv3_confirmed %d, parent %d' % (int(c['conv3_confirmed']), PARENT_CONFIRMED))
    assert c['conv3_confirmed'] == PARENT_CONFIRMED
