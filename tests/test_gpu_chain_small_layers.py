"""GPU: the small layers of the chain kernels (conv0a, conv0b, conv1, conv2 and their epilogues) compute what they computed
before their operand requests and waits were reordered, to the bit.

The existing bit-equality tests compare the screened, the dense and the stem-reusing paths with each other; all of them run
layer_k64 and the epilogues around it, so a change there would move them together.  This test pins them against
tests/golden/chain_small_layers_parent.npz, recorded by tools/make_chain_small_layers_golden.py with the library of the commit
before the reordering: chunks of 3 queries of seeded inputs, per case both pooled STN features, both pooled main features and
the logits, compared with array_equal.

Sizes (patch / sub-sample points): 1 / 40 (a single point; a tile of 40 rows, its second row tile the 16-row tail), 33 / 64
(a 33-row tile; a full tile), 64 / 65 (a full tile; a full tile and a single-point tail tile), 65 / 129, 113 / 200 (several
tiles, tails of 1, 49 and 8 rows).  p2s_max with the default and the adversarial weights, each as three handles (stem reuse on,
off, P2S_CONV3_DENSE=1: the reuse kernel, the save kernel, p2s_chain_kernel<false, true> and the dense kernel); one
sym_op='sum' model (the sum-pool kernel), p2s_vanilla (QSTN short chain and rotation) and one chunk with a NaN coordinate."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import make_chain_small_layers_golden as rec  # noqa: E402

_CACHE = {}


def _golden():
    if 'golden' not in _CACHE:
        with np.load(rec.GOLDEN) as z:
            _CACHE['golden'] = {k: z[k] for k in z.files}
    return _CACHE['golden']


def test_every_case_is_recorded():
    want = {'%s/%s' % (c[0], k) for c in rec.cases() for k in rec.KEYS}
    assert set(_golden()) == want


@pytest.mark.parametrize('case', rec.cases(), ids=lambda c: c[0])
def test_small_layers_equal_the_recorded_parent(case):
    from points2surf_amd import engine, synth
    golden = _golden()
    res = rec.run_case(engine, synth, case, _CACHE.setdefault('weights', {}))
    assert set(res) == {h[0] for h in case[4]}
    for hname, r in res.items():
        for key in rec.KEYS:
            want, got = golden['%s/%s' % (case[0], key)], r[key]
            assert want.shape == got.shape and want.dtype == got.dtype, (case[0], hname, key)
            same = np.array_equal(want, got, equal_nan=True)
            if not same:
                bad = ~((want == got) | (np.isnan(want) & np.isnan(got)))
                print('%s / %s / %s: %d of %d values differ' % (case[0], hname, key, int(bad.sum()), bad.size))
            assert same, (case[0], hname, key)
    if case[5]:
        # the poisoned query's pooled patch feature is NaN in every channel, the other queries are finite
        assert np.isnan(res['reuse']['feat_local'][1]).all()
        assert np.isfinite(res['reuse']['feat_local'][[0, 2]]).all()
