"""Batches over many clouds in one call (engine.CloudSet, p2s_cloudset_*), the validation pass and its losses
(p2s_train_losses, train.validate) and the two loaders of points2surf_amd/train.py.

The yardstick of the set calls is the per-cloud path (Cloud.knn_patch, Rng.subsample_uniform), which the parity suite pins
to the unmodified reference: everything is compared BYTE FOR BYTE, no tolerance.  Three clouds of 700, 1024 and 3,000 points;
the second is scaled by 0.1 and shifted, so the three cell geometries differ and a descriptor mix-up returns visibly wrong
neighbours.  For the sub-sample the sizes matter too: the 1024-point cloud accepts every word of the stream (mask 1023), the
700-point cloud rejects about a third, so segments end at unrelated places of the 624-word blocks -- except where the test
puts an end on a block boundary on purpose (624 ids of the 1024-point cloud from a fresh seed).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import train_model as TM  # noqa: E402

pytestmark = pytest.mark.gpu

CLOUD_OF = [2, 0, 0, 1, 2, 2, 1, 0, 1]
SIZES = (700, 1024, 3000)


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope='module')
def clouds(torch_cuda):
    from points2surf_amd import engine, synth
    pts = [synth.make_cloud(n, seed=i) for i, n in enumerate(SIZES)]
    pts[1] = (pts[1] * np.float32(0.1) + np.array([0.3, -0.2, 0.1], np.float32)).astype(np.float32)
    cl = [engine.Cloud(p) for p in pts]
    cs = engine.CloudSet(cl)
    assert cs.n_clouds == 3 and cs.min_points == 700
    yield pts, cl, cs
    cs.close()
    for c in cl:
        c.close()


def _bits(t):
    """the bytes of a device tensor (float32 compared as bit patterns)"""
    return t.detach().cpu().contiguous().numpy().tobytes()


def _queries(pts):
    """nine queries near the surface of their clouds; item 0 lies 0.3 outside its cloud's box, item 3 IS a cloud point"""
    rs = np.random.default_rng(4)
    q = np.empty((len(CLOUD_OF), 3), np.float32)
    for i, c in enumerate(CLOUD_OF):
        scale = 0.001 if c == 1 else 0.01
        q[i] = pts[c][rs.integers(0, pts[c].shape[0])] + rs.normal(0, scale, 3).astype(np.float32)
    q[0] = pts[2].max(axis=0) + np.array([0.3, 0.0, 0.0], np.float32)
    q[3] = pts[1][5]
    return q


@pytest.mark.parametrize('k', [8, 37, 70])
def test_knn_equals_the_per_cloud_call(clouds, torch_cuda, k):
    pts, cl, cs = clouds
    q = torch_cuda.from_numpy(_queries(pts)).cuda()
    ids, patch, rad = cs.knn_patch(CLOUD_OF, q, k)
    assert ids.shape == (9, k) and patch.shape == (9, k, 3) and rad.shape == (9,)
    for i, c in enumerate(CLOUD_OF):
        ri, rp, rr = cl[c].knn_patch(q[i:i + 1], k)
        assert _bits(ids[i:i + 1]) == _bits(ri), (i, c)
        assert _bits(patch[i:i + 1]) == _bits(rp), (i, c)
        assert _bits(rad[i:i + 1]) == _bits(rr), (i, c)
    assert int(ids[3, 0]) == 5 and float(rad[0]) > 0.3                      # the two special queries are what they claim
    none, patch2, rad2 = cs.knn_patch(np.array(CLOUD_OF, np.int64), q, k, want_ids=False)
    assert none is None and _bits(patch2) == _bits(patch) and _bits(rad2) == _bits(rad)
    ids3, none, rad3 = cs.knn_patch(tuple(CLOUD_OF), q, k, want_patch=False)
    assert none is None and _bits(ids3) == _bits(ids) and _bits(rad3) == _bits(rad)


def _twins(seed, cl, earlier):
    """two generators in the same state: fresh from ``seed``, then ``earlier`` ids drawn on the 3,000-point cloud"""
    from points2surf_amd import engine
    a, b = engine.Rng(seed), engine.Rng(seed)
    if earlier:
        for r in (a, b):
            r.subsample_uniform(cl[2], 1, earlier)
    return a, b


def _check_subsample(torch, cl, cs, cloud_of, S, a, b):
    """the set call on ``a`` against one per-cloud call per item on the twin ``b``: ids, points, generator state"""
    ids, sub = cs.subsample_uniform(a, cloud_of, S)
    assert ids.shape == (len(cloud_of), S) and sub.shape == (len(cloud_of), S, 3)
    for i, c in enumerate(cloud_of):
        ri, rp = b.subsample_uniform(cl[c], 1, S)
        assert int(ri.max()) < SIZES[c]
        assert _bits(ids[i:i + 1]) == _bits(ri), (i, c)
        assert _bits(sub[i:i + 1]) == _bits(rp), (i, c)
    (mt_a, pos_a), (mt_b, pos_b) = a.get_state(), b.get_state()
    assert pos_a == pos_b and np.array_equal(mt_a, mt_b)
    return ids, sub


@pytest.mark.parametrize('earlier', [0, 1000])
@pytest.mark.parametrize('order', ['unsorted', 'sorted'])
def test_subsample_equals_the_per_cloud_sequence(clouds, torch_cuda, order, earlier):
    pts, cl, cs = clouds
    cloud_of = CLOUD_OF if order == 'unsorted' else sorted(CLOUD_OF)
    a, b = _twins(17, cl, earlier)
    _check_subsample(torch_cuda, cl, cs, cloud_of, 53, a, b)
    _check_subsample(torch_cuda, cl, cs, cloud_of, 53, a, b)               # and again from where that left the stream
    a.close()
    b.close()


def test_subsample_segment_ends_on_a_block_boundary(clouds, torch_cuda):
    """624 ids of the 1024-point cloud from a fresh seed are exactly the first 624-word block: the second item starts
    behind a twist"""
    pts, cl, cs = clouds
    a, b = _twins(23, cl, 0)
    probe, _ = _twins(23, cl, 0)
    probe.subsample_uniform(cl[1], 1, 624)
    assert probe.get_state()[1] == 624
    probe.close()
    _check_subsample(torch_cuda, cl, cs, [1, 0, 2, 1], 624, a, b)
    a.close()
    b.close()


def test_subsample_after_a_session(clouds, torch_cuda):
    """a per-cloud call large enough to open a session of the parallel generator, then the set call: it closes the session
    and goes on from there like the per-cloud sequence"""
    pts, cl, cs = clouds
    a, b = _twins(29, cl, 0)
    for r in (a, b):
        r.subsample_uniform(cl[2], 400, 1000, want_pts=False)
    _check_subsample(torch_cuda, cl, cs, CLOUD_OF, 53, a, b)
    a.close()
    b.close()


def test_subsample_skip_and_repeat(clouds, torch_cuda):
    pts, cl, cs = clouds
    a, b = _twins(31, cl, 1000)
    mt0, pos0 = a.get_state()
    ids, sub = cs.subsample_uniform(a, CLOUD_OF, 53)
    cs.skip(b, CLOUD_OF, 53)
    (mt_a, pos_a), (mt_b, pos_b) = a.get_state(), b.get_state()
    assert pos_a == pos_b and np.array_equal(mt_a, mt_b)
    assert pos_a != pos0 or not np.array_equal(mt_a, mt0)
    a.set_state(mt0, pos0)
    ids2, sub2 = cs.subsample_uniform(a, CLOUD_OF, 53)
    assert _bits(ids2) == _bits(ids) and _bits(sub2) == _bits(sub)
    ids3, none = cs.subsample_uniform(b, CLOUD_OF, 53, want_pts=False)     # ids alone; b is one call further
    assert none is None and _bits(ids3) != _bits(ids)
    a.close()
    b.close()


def test_refusals_name_the_item(clouds, torch_cuda):
    from points2surf_amd import engine, _lib
    pts, cl, cs = clouds
    q = torch_cuda.from_numpy(_queries(pts)).cuda()
    r = engine.Rng(1)
    before = r.get_state()
    bad = list(CLOUD_OF)
    bad[4] = 3
    with pytest.raises(_lib.P2SError, match='item 4 names cloud 3'):
        cs.knn_patch(bad, q, 8)
    with pytest.raises(_lib.P2SError, match='item 4 names cloud 3'):
        cs.subsample_uniform(r, bad, 53)
    with pytest.raises(_lib.P2SError, match='item 1: cloud 0 has 700 points < k=701'):
        cs.knn_patch(CLOUD_OF, q, 701)
    with pytest.raises(_lib.P2SError, match='item 1: cloud 0 has 700 points < n=701'):
        cs.subsample_uniform(r, CLOUD_OF, 701)
    with pytest.raises(_lib.P2SError, match='item 0 names cloud -1'):
        cs.knn_patch([-1], q[:1], 8)
    with pytest.raises(ValueError):
        cs.knn_patch(CLOUD_OF[:3], q, 8)
    after = r.get_state()
    assert before[1] == after[1] and np.array_equal(before[0], after[0])   # a refused call draws nothing
    ids, patch, rad = cs.knn_patch([], q[:0], 8)                            # no items: fine, no launch
    assert ids.shape == (0, 8) and rad.shape == (0,)
    ids, sub = cs.subsample_uniform(r, [], 53)
    assert ids.shape == (0, 53) and sub.shape == (0, 53, 3)
    ids, _, _ = cs.knn_patch([0], q[1:2], 700)                              # k = the whole cloud is allowed
    assert sorted(ids[0].tolist()) == list(range(700))
    r.close()


# -- the losses of given predictions ----------------------------------------------------------------------------------------
def _losses64(pred, dist_abs, sign01, radius):
    """the two formulas of p2s_train_loss_kernel in float64, the target ratio in float32 first as the kernel has it"""
    p0, p1 = pred[:, 0].astype(np.float64), pred[:, 1].astype(np.float64)
    t = np.tanh(np.abs((dist_abs.astype(np.float32) / radius.astype(np.float32)).astype(np.float64)))
    mag = np.mean((np.tanh(np.abs(p0)) - t) ** 2)
    y = sign01.astype(np.float64)
    sgn = np.mean(np.maximum(p1, 0.0) - p1 * y + np.log1p(np.exp(-np.abs(p1))))
    return float(mag), float(sgn)


@pytest.mark.parametrize('B', [1, 2, 257, 1000])
def test_train_losses(torch_cuda, B):
    from points2surf_amd import train
    b = TM.make_batch(B, 1, 1, seed=100 + B)
    pred = np.random.default_rng(B).uniform(-8, 8, (B, 2)).astype(np.float32)
    dev = [torch_cuda.from_numpy(a).cuda() for a in (pred, b['dist_abs'], b['sign01'], b['radius'])]
    got = train.losses(*dev)
    ref = _losses64(pred, b['dist_abs'], b['sign01'], b['radius'])
    print('B = %d: device %r, float64 %r' % (B, got, ref))
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-10 * abs(r), (B, got, ref)


# -- a small data set on disk, shared ----------------------------------------------------------------------------------------
P, S, BATCH, PPS = 16, 32, 8, 16


@pytest.fixture(scope='module')
def dataset(tmp_path_factory, torch_cuda):
    """three stand-in shapes of 1,200 points with 24 query points each; the same list serves as training and test set"""
    from points2surf_amd import synth
    root = str(tmp_path_factory.mktemp('loader_data'))
    names = synth.make_standin_dataset(root, [synth.make_cloud(1200, seed=0), synth.make_cloud(1200, seed=1, kind='sphere')], 3,
                                       list_name='trainset.txt')
    with open(os.path.join(root, 'testset.txt'), 'w') as f:
        f.write('\n'.join(names) + '\n')
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, '05_query_pts'))
    os.makedirs(os.path.join(root, '05_query_dist'))
    for n in names:
        pts = np.load(os.path.join(root, '04_pts', n + '.xyz.npy'))
        q = (pts[rng.integers(0, pts.shape[0], 24)] + rng.normal(0, 0.02, (24, 3))).astype(np.float32)
        np.save(os.path.join(root, '05_query_pts', n + '.ply.npy'), q)
        np.save(os.path.join(root, '05_query_dist', n + '.ply.npy'), rng.normal(0, 0.02, 24).astype(np.float32))
    return root


def _options(root, outdir, name, extra=()):
    from points2surf_amd import train
    return train.parse_arguments(['--indir', root, '--name', name, '--outdir', outdir, '--nepoch', '2', '--batchSize', str(BATCH),
                                  '--patches_per_shape', str(PPS), '--points_per_patch', str(P), '--sub_sample_size', str(S),
                                  '--scheduler_steps', '1', '--seed', '3'] + list(extra))


@pytest.mark.parametrize('loader', ['per_shape', 'set'])
@pytest.mark.parametrize('name', ['p2s_max', 'p2s_max_no_feat_stn'])
def test_validate_against_the_cpu_forward(dataset, torch_cuda, tmp_path, name, loader):
    """the batches assembled here through the per-cloud calls with a twin Rng(seed + 1), the CPU forward of the oracle, the two
    losses in float64.  Gate: the project's 1e-4 logit contract (test_gpu_train: |logits - oracle| < 1e-4) times the
    Lipschitz constants of the two losses (train_model.loss_gates: 2 and 1), plus the rounding of the loss itself.  15 patches
    per shape: 45 items, five batches of 8 and a short one of 5."""
    from points2surf_amd import engine, synth, train
    from oracle import torch_port, p2s_oracle
    w, cfg = synth.make_weights(name)
    cfg = dict(cfg, points_per_patch=P, sub_sample_size=S)
    opt = _options(dataset, str(tmp_path), 'v', ['--patches_per_shape', '15', '--use_feat_stn', str(int(cfg['use_feat_stn'])),
                                                '--loader', loader])
    dev = engine.select_device(0)
    data = train.TrainData.load(dataset, 'testset.txt', P, S, dev)
    got = train.validate(w, opt, data, dev)
    again = train.validate(w, opt, data, dev)
    assert got == again                                                     # every pass sees identical batches
    # the oracle
    order = train.epoch_order(data.n_queries, 15, opt.seed, -1)
    assert order.shape[0] == 45
    rng = engine.Rng(opt.seed + 1, dev)
    sums, batches = np.zeros(2), 0
    for b0 in range(0, 45, BATCH):
        items = order[b0:b0 + BATCH]
        items = items[np.argsort(items[:, 0], kind='stable')]
        patch, sub, rad, q, d = [], [], [], [], []
        for s, qi in items:
            one = data.queries[data.offsets[s] + qi][None, :]
            _, p, r = data.clouds[s].knn_patch(torch_cuda.from_numpy(one).cuda(), P, want_ids=False)
            patch.append(p.cpu().numpy())
            rad.append(r.cpu().numpy())
            sub.append(rng.subsample_uniform(data.clouds[s], 1, S)[1].cpu().numpy())
            q.append(one)
            d.append(data.dists[data.offsets[s] + qi])
        patch, sub, rad, q, d = np.concatenate(patch), np.concatenate(sub), np.concatenate(rad), np.concatenate(q), np.array(d, np.float32)
        if cfg['use_feat_stn']:
            logits = torch_port.TorchPort(w, cfg).forward(patch, sub, q).numpy()
        else:
            logits = p2s_oracle.model_forward(w, cfg, patch, sub, q)
        sums += _losses64(logits, np.abs(d), (d >= 0).astype(np.float32), rad)
        batches += 1
    rng.close()
    data.close()
    assert batches == 6
    ref = sums / batches
    gates = [2e-4 + 4 * 2.0 ** -24 * abs(ref[0]), 1e-4 + 4 * 2.0 ** -24 * abs(ref[1])]
    print('%s, loader %s: validation %r, oracle %r, gates %r' % (name, loader, got, tuple(ref), gates))
    assert np.isfinite(got).all()
    for g, r, t in zip(got, ref, gates):
        assert abs(g - r) <= t, (got, tuple(ref), gates)


def _checkpoint_bytes(torch, path):
    sd = torch.load(path, map_location='cpu', weights_only=False)
    return {k: v.numpy().tobytes() for k, v in sd.items()}


def test_loaders_write_equal_checkpoints_and_validation_leaves_training_alone(dataset, torch_cuda, tmp_path, capsys):
    import re
    from points2surf_amd import train
    out = str(tmp_path)
    files = {}
    for tag, extra in (('a', ['--loader', 'per_shape']), ('b', ['--loader', 'set']),
                       ('c', ['--loader', 'set', '--testset', 'testset.txt'])):
        capsys.readouterr()
        files[tag] = train.train(_options(dataset, out, tag, extra))
        text = capsys.readouterr().out
        lines = [l for l in text.splitlines() if l.startswith('epoch')]
        assert len(lines) == 2 and text.count('epoch') == 2, text
        for l in lines:
            val = re.findall(r'validation: magnitude loss ([-0-9.einfa]+), sign loss ([-0-9.einfa]+)', l)
            if tag == 'c':
                assert len(val) == 1 and np.isfinite([float(v) for v in val[0]]).all(), l
            else:
                assert not val and 'validation' not in l, l
    ref = _checkpoint_bytes(torch_cuda, files['a'])
    assert len(ref) > 100 and int(torch_cuda.load(files['a'], weights_only=False)['module.bn2.num_batches_tracked']) == 12
    for tag in ('b', 'c'):
        got = _checkpoint_bytes(torch_cuda, files[tag])
        assert list(got) == list(ref)
        for k in ref:
            assert got[k] == ref[k], (tag, k)
    saved = torch_cuda.load(os.path.join(out, 'c_params.pth'), weights_only=False)
    assert saved.loader == 'set' and saved.testset == 'testset.txt'


def test_set_loader_names_a_cloud_that_is_too_small(dataset, torch_cuda, tmp_path):
    from points2surf_amd import train
    with pytest.raises(ValueError, match=r"shape \S+ has 1200 points"):
        train.train(_options(dataset, str(tmp_path), 'd', ['--loader', 'set', '--sub_sample_size', '1201']))
