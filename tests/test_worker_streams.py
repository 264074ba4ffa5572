"""Workers mode, host side (no GPU): the stream model of points2surf_amd/streams.py against a brute-force order, and
against the per-batch sub-sample digests the unmodified reference's DataLoader produced with --workers 3 --batchSize 37
(tests/golden/ref_workers_p2s_max_w3_b37.npz, tools/make_golden_workers.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

from points2surf_amd import streams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
SEED = 40938661

# (g0, n, W, B): B = 1, B >= n, g0 inside a batch, one stream, the shipped command line, empty
PARAMS = [(0, 1000, 7, 501), (0, 50, 3, 1), (0, 100, 4, 1000), (10, 100, 4, 100), (37 * 5 + 11, 2000, 3, 37),
          (0, 1, 1, 1), (1234, 777, 1, 50), (501 * 7 * 3 + 250, 4000, 7, 501), (5, 0, 3, 4), (2 ** 40 + 3, 300, 5, 17)]


def brute_force(g0, n, W, B):
    key = [((g // B) % W, g) for g in range(g0, g0 + n)]
    order = sorted(range(n), key=lambda i: key[i])
    counts = [sum(1 for k in key if k[0] == w) for w in range(W)]
    return np.array(order, np.int64), np.array(counts, np.int64)


@pytest.mark.parametrize('g0,n,W,B', PARAMS)
def test_stream_order_matches_brute_force(g0, n, W, B):
    order, counts = streams.stream_order(g0, n, W, B)
    o_ref, c_ref = brute_force(g0, n, W, B)
    assert order.dtype == np.int64 and counts.dtype == np.int64
    assert np.array_equal(order, o_ref)
    assert np.array_equal(counts, c_ref)


def test_stream_order_random_parameters():
    rng = np.random.default_rng(7)
    for _ in range(300):
        g0, n, W, B = int(rng.integers(0, 10 ** 6)), int(rng.integers(0, 400)), int(rng.integers(1, 9)), int(rng.integers(1, 120))
        order, counts = streams.stream_order(g0, n, W, B)
        o_ref, c_ref = brute_force(g0, n, W, B)
        assert np.array_equal(order, o_ref) and np.array_equal(counts, c_ref), (g0, n, W, B)


def test_one_stream_and_one_batch_are_the_identity():
    for g0, n, W, B in [(0, 500, 1, 37), (100, 500, 7, 10 ** 6), (0, 501, 7, 501)]:
        order, counts = streams.stream_order(g0, n, W, B)
        assert np.array_equal(order, np.arange(n))
        assert counts.sum() == n
    assert np.array_equal(streams.stream_of([0, 36, 37, 74, 111, 112], 3, 37), [0, 0, 1, 2, 0, 0])
    with pytest.raises(ValueError):
        streams.stream_of([0], 0, 5)


def _golden(name):
    path = os.path.join(GOLDEN, 'ref_workers_%s.npz' % name)
    with open(os.path.join(GOLDEN, 'meta_workers.json')) as f:
        meta = json.load(f)['ref_workers_' + name]
    return np.load(path), meta


def abc3_queries(meta, res=32):
    """the abc3 clouds and their query grids in dataset order (checked against the golden's query hashes)"""
    from oracle import p2s_oracle as po
    clouds, grids = [], []
    for sh in meta['shapes']:
        pts = np.load(os.path.join(GOLDEN, 'abc_minimal', '04_pts', sh['name'] + '.xyz.npy')).astype(np.float32)[:, :3]
        q = po.query_grid(pts, res, 3)[0]
        assert q.shape[0] == sh['queries']
        assert hashlib.sha256(np.ascontiguousarray(q).tobytes()).hexdigest() == sh['query_sha256']
        clouds.append(pts)
        grids.append(q)
    return clouds, grids


def test_reference_batches_rebuilt_from_stream_twins():
    """p2s_max (uniform sub-sample), --workers 3 --batchSize 37: every batch's sub-sample digest of the reference's
    DataLoader, rebuilt from three LegacyMT19937(seed) twins, each consuming its own queries in dataset order"""
    from oracle import p2s_oracle as po
    g, meta = _golden('p2s_max_w3_b37')
    W, B = meta['workers'], meta['batchSize']
    assert (W, B) == (3, 37) and meta['self_check']['batches_rebuilt'] == len(g['sub_sha'])
    clouds, grids = abc3_queries(meta)
    shape_of = np.concatenate([np.full(q.shape[0], s) for s, q in enumerate(grids)])
    local = np.concatenate([np.arange(q.shape[0]) for q in grids])
    total = shape_of.size
    order, counts = streams.stream_order(0, total, W, B)
    pts = np.empty((total, 1000, 3), np.float32)
    at = 0
    for w in range(W):
        rng = po.LegacyMT19937(SEED)
        for i in order[at:at + counts[w]]:
            s = shape_of[i]
            pts[i] = po.subsample_points(rng, clouds[s], grids[s][local[i]], 1000, uniform=True)
        at += counts[w]
    sizes = g['batch_sizes']
    assert sizes.sum() == total
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for b in range(len(sizes)):
        got = hashlib.sha256(pts[starts[b]:starts[b + 1]].tobytes()).digest()
        assert got == g['sub_sha'][b].tobytes(), 'batch %d (worker %d)' % (b, b % W)
