"""CPU: the adversarial weight sets (synth.STRESS_MODELS: BatchNorm gamma of both signs and near zero, running_var down to
1e-6, unscaled STN / QSTN fc3, all-zero conv rows) -- the numpy oracle in fp32 and float64 against the goldens of the
unmodified reference (oracle/make_golden_stress.py) under the conditioned bound of points2surf_amd/parity.py; power checks
that show the comparison can fail (an oracle that pools before the bn3 affine, or drops trans2 / the QSTN rotation, misses
by far more than the bound); the sets' statistics; the fp16-pair arithmetic model's loss below fp16's normal range."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import p2s_oracle as O
from points2surf_amd import parity, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# sha256 over (name, bytes) of every array of the named synthetic sets, in key order: every committed golden depends on them
_SHA = {
    'p2s_large_kNN': 'f6cafe984d814a553283df09e6ca7b6a8cf40dfb4de2cf0fa8eec23176cb98fc',
    'p2s_large_radius': '1b494bbe53c65154c8664fa5d23c15a6cf2e98831d28440cc9ee8547a6e1e783',
    'p2s_max': '2cb0925dae21d94a9f6b4c7d2b5328bf83d191c019248961167886f93c805ced',
    'p2s_max_no_feat_stn': '39d06a3134bc2a31873a9157eaf52f56e174ffe2eb1f1c6ca6848c69e6129e8e',
    'p2s_max_sum': '885f07b4afbc663d7d54cf4708384c965a61584530f560ed5caf9db2e1f56b1d',
    'p2s_medium_radius': 'd214a06d54e081ee5544c9a9a546dbc2dd82cfaaff61a55f13da6d10ba7dab56',
    'p2s_no_qstn': '8146453b82d8a2e97fcf2a731dfeaa7a6f0305a7751bd4590fae26709b7ac364',
    'p2s_regression': '2881a80b6d7ce8e4a5e5734b273e33ef31f52867d47ac5744c58338aac4271d3',
    'p2s_shared_encoder': '61ec25c42efe8e7f752fb36c95b55d0d0ed4577c6643b99e1f9cee9d17536ca8',
    'p2s_shared_encoder_sum': '6a42f48026103d28a0e96f0ec865504669f57f58a54fe2a0636ab5c3f876e67d',
    'p2s_small_kNN': '748bcdb5552da25203b608178362b3ea69c3fdf3fc0126d543f0fa6c64a3a61b',
    'p2s_small_radius': '848223d1f0a6eec9ad3614ebcc97ceb46ba02402f20c67d71811e5420377a36d',
    'p2s_uniform': 'faa1af9c1b0f15eadb7efcf4efa4accce03b97201cf468708ec63c39f5650d3a',
    'p2s_vanilla': '527bdab97255c911919c404164cd19992ae5eb362724cab60dae0365ddd44e00',
    'p2s_vanilla_mixed': '1deea624fd19d6cddaf8b573e1bf27f5b3d30f98f6474a42a7b9753506615d34',
}


def _weights_sha(w):
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
    return h.hexdigest()


def test_named_sets_unchanged_and_stress_sets_derived():
    for name, digest in _SHA.items():
        assert _weights_sha(synth.make_weights(name)[0]) == digest, name
    for name in synth.STRESS_MODELS:
        w, cfg = synth.make_weights(name)
        base, cfg0 = synth.make_weights(name.replace('_stress', ''))
        assert cfg == cfg0 and sorted(w) == sorted(base)
        assert all(w[k].dtype == base[k].dtype and w[k].shape == base[k].shape for k in w)
        assert _weights_sha(synth.make_weights(name)[0]) == _weights_sha(w)        # reproducible


def stress_evals(model, cloud, step=1):
    """the recorded queries of a stress golden (every ``step``-th) with their network inputs and the logits of: the
    reference (golden), the float64 oracle, the fp32 oracle, the fp32 oracle in reversed summation order"""
    path = os.path.join(GOLDEN, 'ref_stress_%s.npz' % model)
    if not os.path.isfile(path):
        pytest.fail('golden missing: %s' % path)
    g = dict(np.load(path))
    sel = np.arange(0, g['query_index'].shape[0], step)
    q = np.load(os.path.join(GOLDEN, 'query_grid_32_3.npy'))[g['query_index'][sel]]
    knn, sub_ids = g['knn_ids'][sel], g['sub_ids'][sel]
    r, ps = O.patch_radius_and_ps(cloud, knn, q)
    sub = cloud[sub_ids]
    w, cfg = synth.make_weights(model)
    f64, fl, fg = O.model_forward(w, cfg, ps, sub, q, dtype=np.float64, return_feats=True)
    return {'w': w, 'cfg': cfg, 'g': g, 'sel': sel, 'q': q, 'knn': knn, 'sub_ids': sub_ids, 'ps': ps, 'sub': sub, 'r': r,
            'ref': g['logits'][sel], 'f64': f64, 'feat64': (fl, fg),
            'f32': O.model_forward(w, cfg, ps, sub, q), 'f32r': O.model_forward(w, cfg, ps, sub, q, rev=True)}


def bound_of(e, encoder_bf16=0):
    """THE conditioned bound of the stress tests (parity.conditioned_bound over the three fp32 evaluations)"""
    return parity.conditioned_bound(e['f64'], [e['ref'], e['f32'], e['f32r']], encoder_bf16=encoder_bf16)


_CACHE = {}


def _evals(model, cloud):
    if model not in _CACHE:
        _CACHE[model] = stress_evals(model, cloud, step=2)       # 64 of the 128 recorded queries: the CPU suite's time budget
    return _CACHE[model]


@pytest.mark.parametrize('model', synth.STRESS_MODELS)
def test_oracles_match_the_reference_under_the_conditioned_bound(model, fixture_cloud):
    e = _evals(model, fixture_cloud)
    assert np.array_equal(e['r'], e['g']['radius'][e['sel']])
    b = bound_of(e)
    spread = (b - parity.COND_FLOOR_FP32) / parity.COND_FACTOR
    print('%s: fp32 spread around float64: median %.3g, max %.3g; |ref - f64| max %.3g' % (
        model, float(np.median(spread)), float(spread.max()), float(np.abs(e['ref'] - e['f64']).max())))
    for key in ('ref', 'f32', 'f32r'):
        assert float(parity.conditioned_excess(e[key], e['f64'], b).max()) <= 1.0, key
    # post-processing: the float64 SDF of the float64 logits against that of the reference's logits
    sdf64 = O.post_process(e['f64'], e['r'], dtype=np.float64)
    sdf = O.post_process(e['ref'], e['r'])
    near = np.abs(e['f64'][:, 1]) < b[:, 1]
    assert np.all(np.sign(sdf[~near]) == np.sign(sdf64[~near]))
    assert float(np.abs(np.abs(sdf) - np.abs(sdf64)).max()) < 1e-5


def _feat_pool_before_affine(x, w, pre, use_point_stn, use_feat_stn=True, return_aux=False, sym_op='max', rev=False):
    """pointnetfeat_forward with the max-pool taken BEFORE the bn3 affine (the mistake a kernel that pooled the raw conv3
    output and applied the folded scale afterwards would make; right only for gamma > 0)"""
    trans = None
    if use_point_stn:
        trans, _ = O.qstn_forward(x, w, pre + '.stn1')
        x = np.einsum('bij,bpj->bpi', trans, x)
    x = O._relu(O._bn(O._conv(x, w, pre + '.conv0a'), w, pre + '.bn0a', 2))
    x = O._relu(O._bn(O._conv(x, w, pre + '.conv0b'), w, pre + '.bn0b', 2))
    if use_feat_stn:
        x = np.einsum('bij,bpj->bpi', O.stn_forward(x, w, pre + '.stn2', 64), x)
    x = O._relu(O._bn(O._conv(x, w, pre + '.conv1'), w, pre + '.bn1', 2))
    x = O._relu(O._bn(O._conv(x, w, pre + '.conv2'), w, pre + '.bn2', 2))
    x = O._bn(O._conv(x, w, pre + '.conv3').max(axis=1), w, pre + '.bn3', 1)
    return x, trans


def _identity_stn(x, w, pre, dim, rev=False):
    return np.broadcast_to(np.eye(dim, dtype=x.dtype), (x.shape[0], dim, dim))


def _identity_qstn(x, w, pre, rev=False):
    quat = np.zeros((x.shape[0], 4), x.dtype)
    quat[:, 0] = 1
    return np.broadcast_to(np.eye(3, dtype=x.dtype), (x.shape[0], 3, 3)), quat


_BROKEN = [('p2s_max_stress', 'pointnetfeat_forward', _feat_pool_before_affine),
           ('p2s_vanilla_stress', 'pointnetfeat_forward', _feat_pool_before_affine),
           ('p2s_max_stress', 'stn_forward', _identity_stn),
           ('p2s_vanilla_stress', 'qstn_forward', _identity_qstn)]


@pytest.mark.parametrize('model,fn,broken', _BROKEN, ids=['%s-%s' % (m, b.__name__) for m, _, b in _BROKEN])
def test_power_a_wrong_oracle_misses_by_far_more_than_the_bound(model, fn, broken, fixture_cloud, monkeypatch):
    e = _evals(model, fixture_cloud)
    b = bound_of(e, encoder_bf16=4)                       # the loosest bound any mode is held to
    monkeypatch.setattr(O, fn, broken)
    n = 32
    lg = O.model_forward(e['w'], e['cfg'], e['ps'][:n], e['sub'][:n], e['q'][:n])
    ex = parity.conditioned_excess(lg, e['f64'][:n], b[:n]).max(axis=1)
    print('%s / %s: median excess %.3g, share of queries > 100x the bound %.2f' % (
        model, broken.__name__, float(np.median(ex)), float((ex > 100).mean())))
    assert (ex > 100).mean() >= 0.5


@pytest.mark.parametrize('model', synth.STRESS_MODELS)
def test_stress_statistics(model):
    with open(os.path.join(GOLDEN, 'meta_stress.json')) as f:
        st = json.load(f)[model]
    from oracle.make_golden_stress import weight_stats
    w, _ = synth.make_weights(model)
    assert weight_stats(w) == {k: st[k] for k in weight_stats(w)}        # the recorded statistics are those of these weights
    assert 0.3 <= st['gamma_negative_frac'] <= 0.5 and 0.03 <= st['gamma_tiny_frac'] <= 0.07 and st['gamma_zero_count'] > 0
    assert st['running_var_min'] < 2e-6 and st['running_var_max'] > 5 and st['zero_conv_rows'] > 0
    assert st['trans2_minus_I_max'] > 10
    assert 0.2 <= st['sign_logit_pos_frac'] <= 0.8 and 0.2 <= st['sdf_pos_frac_grid32'] <= 0.8
    assert st['tanh2_below_0p9_frac'] > 0.5
    if 'quat_sumsq_min' in st:
        assert st['quat_sumsq_min'] < 0.3 and st['quat_sumsq_in_0p05_0p3'] >= 5
    assert model != 'p2s_vanilla_stress' or 'quat_sumsq_min' in st


def test_fp16_pair_model_loses_precision_below_the_normal_range():
    """the split x = h0 + h1 2^-11 of test_fp16_pair_model: 22 bits down to 2^-14, then an absolute floor of ~2^-36 --
    the loss the fp16-pair encoder's rebalancing (points2surf_amd/weights.py: _balance) exists for"""
    from test_fp16_pair_model import _split16
    g = np.random.default_rng(5)
    err = {}
    for k in (0, 8, 14, 18, 24, 32):
        x = (g.uniform(0.5, 1.0, 20000) * 2.0 ** -k).astype(np.float32)
        h0, h1 = _split16(x)
        y = h0.astype(np.float64) + h1.astype(np.float64) / 2048.0
        err[k] = float((np.abs(y - x) / x).max())
        assert float(np.abs(y - x).max()) <= 2.0 ** -23 * 2.0 ** -k + 2.0 ** -35
    assert err[0] < 2.5e-7 and err[8] < 2.5e-7                # normal range: 22-23 bits
    assert err[18] > 20 * err[0] and err[24] > 1e-4 and err[32] > 1e-2
