"""Host model of the reference's multi-worker sub-sample streams (``--workers W --batchSize B``).

torch's map-style DataLoader hands batch b -- dataset positions [b B, (b+1) B) of the sampler's sequence, across shape
boundaries -- to worker b mod W, and every worker holds its own copy of the dataset, so of both
``np.random.RandomState(seed)`` generators (reference source/data_loader.py:270-277).  The query at dataset position g
therefore draws from worker stream ``(g // B) mod W``; each stream consumes its own queries in increasing g.

Pure numpy.  The device kernel behind ``p2s_stream_order`` computes the same permutation; the tests use this module as
its reference.
"""
import numpy as np


def stream_of(positions, W, B):
    """worker stream of every dataset position: (g // B) mod W"""
    W, B = int(W), int(B)
    if W < 1 or B < 1:
        raise ValueError('workers and batch size must be >= 1 (got %d, %d)' % (W, B))
    return (np.asarray(positions, dtype=np.int64) // B) % W


def stream_order(g0, n, W, B):
    """the stream-major permutation of the local queries 0..n-1 at positions g0..g0+n-1: stream 0's queries in
    increasing position, then stream 1's, ...  Returns (order [n] int64, counts [W] int64)."""
    g0, n = int(g0), int(n)
    if g0 < 0 or n < 0:
        raise ValueError('bad range g0=%d n=%d' % (g0, n))
    w = stream_of(np.arange(g0, g0 + n, dtype=np.int64), W, B)
    order = np.argsort(w, kind='stable').astype(np.int64)
    counts = np.bincount(w, minlength=int(W)).astype(np.int64)
    return order, counts
