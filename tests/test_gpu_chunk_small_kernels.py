"""GPU: the kernels a chunk runs around its two chain launches -- the FC layers of the STN head and of the decoder, the fold, the
decoder tail -- compute what they computed before the FC kernel was re-pipelined, to the bit.

tests/golden/chunk_small_kernels_parent.npz was recorded by tools/make_chunk_small_kernels_golden.py with the library of the
commit before the change: chunks of 130, 3, 1 and 2050 grid queries of the fixture cloud (130 = four 32-row tiles and a ragged
fifth of 2 rows; 1 = one row; 2050 = the 64-row kernel for the 4096-column layer, 32 full tiles and a ragged one of 2 rows), per
case the pooled STN features, both pooled main features, the logits and the SDF.  Weight sets: p2s_max default and adversarial, each with stem reuse on and off (the two must agree with
each other and with the file); p2s_vanilla (QSTN head); a sym_op='sum' model; the two single_transformer models (the FC kernel's
second operand, as max and as sum); p2s_max with the fp16-pair encoder (16-bit head layers, untouched); one chunk with a NaN
coordinate.  Everything is compared with array_equal (NaN = NaN); the wide arrays of the larger chunks through the SHA-256 of
their canonical bytes, which is equal exactly when array_equal holds (the arrays themselves would not fit a committed file)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import make_chunk_small_kernels_golden as rec  # noqa: E402

_CACHE = {}


def _golden():
    if 'golden' not in _CACHE:
        with np.load(rec.GOLDEN) as z:
            _CACHE['golden'] = {k: z[k] for k in z.files}
    return _CACHE['golden']


def test_every_case_is_recorded_and_the_inputs_are_the_recorded_ones():
    from points2surf_amd import engine
    want = {'%s/%s' % (c[0], k) for c in rec.cases() for k in rec.KEYS} | {'inputs/%d' % i for i in range(4)}
    assert set(_golden()) == want
    for i, t in enumerate(rec.inputs(engine, _CACHE)):
        assert np.array_equal(_golden()['inputs/%d' % i], rec.digest(t.cpu().numpy())), 'network input %d differs from the recorded one' % i


@pytest.mark.parametrize('case', rec.cases(), ids=lambda c: c[0])
def test_chunk_outputs_equal_the_recorded_parent(case):
    from points2surf_amd import engine, synth
    golden = _golden()
    res = rec.run_case(engine, synth, case, _CACHE)
    assert set(res) == {h[0] for h in case[4]}
    for hname, r in res.items():
        for key in rec.KEYS:
            want, got = golden['%s/%s' % (case[0], key)], rec.recorded(case, key, r[key])
            assert want.shape == got.shape and want.dtype == got.dtype, (case[0], hname, key)
            same = np.array_equal(want, got, equal_nan=got.dtype.kind == 'f')
            if not same and got.dtype.kind == 'f':
                bad = ~((want == got) | (np.isnan(want) & np.isnan(got)))
                print('%s / %s / %s: %d of %d values differ' % (case[0], hname, key, int(bad.sum()), bad.size))
            assert same, (case[0], hname, key)
    if case[5]:
        # the poisoned query: NaN logits, SDF 1.0 (the reference's NaN rule); its neighbours in the row tile are finite
        r = res[case[4][0][0]]
        assert np.isnan(r['logits'][77]).all() and r['sdf'][77] == 1.0
        assert np.isnan(r['feat_local'][77]).all()
        ok = np.arange(case[3]) != 77
        assert np.isfinite(r['logits'][ok]).all() and np.isfinite(r['sdf'][ok]).all() and np.isfinite(r['feat_local'][ok]).all()


def test_rows_do_not_depend_on_the_chunk_they_run_in():
    """a query's outputs are the same floats as row 0 of a 1-query chunk, in a 3-query chunk, a 130-query chunk and a
    2050-query chunk: the row tile a row falls into (full, ragged, 32 or 64 rows) does not enter its accumulation chains"""
    from points2surf_amd import engine, synth
    by_nq = {c[3]: rec.run_case(engine, synth, c, _CACHE)['reuse'] for c in rec.cases() if c[1] == 'p2s_max' and not c[2] and not c[5]}
    for key in rec.KEYS:
        def rows(a, n):
            return a[:, :n] if key == 'stn_pool' else a[:n]          # stn_pool is [encoder][query][channel]
        assert np.array_equal(by_nq[1][key], rows(by_nq[3][key], 1)), key
        assert np.array_equal(by_nq[3][key], rows(by_nq[rec.NQ][key], 3)), key
        assert np.array_equal(by_nq[rec.NQ][key], rows(by_nq[rec.NBIG][key], rec.NQ)), key
