"""The training entry points are part of the C ABI (CPU: symbols, prototypes and refusals that need no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRAINER_SYMBOLS = ['p2s_trainer_copy_out', 'p2s_trainer_create', 'p2s_trainer_destroy', 'p2s_trainer_forward_backward',
                   'p2s_trainer_pool_indices', 'p2s_trainer_profile', 'p2s_trainer_sgd_step', 'p2s_trainer_sizes']


@pytest.fixture(scope='module')
def lib():
    from points2surf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_trainer_symbols_declared_bound_and_exported(lib):
    from points2surf_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'p2s_hip.h')).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(p2s_trainer_[a-z0-9_]+)\s*\(', src)))
    assert declared == TRAINER_SYMBOLS
    for s in TRAINER_SYMBOLS:
        assert s in _lib.PROTOTYPES and hasattr(lib, s), s
    assert 'typedef struct p2s_trainer_s *p2s_trainer_t;' in src


def test_abi_version_is_still_5(lib):
    assert lib.p2s_abi_version() == 5


def test_flat_layout_matches_state_shapes(lib):
    """the library checks the sizes of the flat arrays before it looks for a device: right sizes pass that check, wrong
    ones are named"""
    from points2surf_amd import model_spec, weights
    for stn, n_p, n_b in ((1, None, None), (0, None, None)):
        shapes = model_spec.state_shapes(use_feat_stn=bool(stn))
        n_p = sum(int(np.prod(s)) for k, s in shapes.items() if k.endswith(('.weight', '.bias')))
        n_b = sum(int(np.prod(s)) for k, s in shapes.items() if k.endswith(('.running_mean', '.running_var')))
        mc = weights.ModelCfg(net_size=1024, points_per_patch=8, sub_sample_size=8, output_dim=2)
        p, b = np.zeros(n_p + 1, np.float32), np.zeros(n_b, np.float32)
        h = ctypes.c_void_p()
        rc = lib.p2s_trainer_create(ctypes.byref(mc), stn, p.ctypes.data_as(ctypes.c_void_p), n_p + 1,
                                    b.ctypes.data_as(ctypes.c_void_p), n_b, 0, 0, ctypes.byref(h))
        assert rc == -1 and (b'%d / %d' % (n_p, n_b)) in lib.p2s_last_error(), lib.p2s_last_error()


@pytest.mark.parametrize('field,value,word', [
    ('use_point_stn', 1, b'QSTN'), ('single_transformer', 1, b'shared encoder'), ('shared_transformer', 1, b'shared transformer'),
    ('sym_sum', 1, b'sum pooling'), ('output_dim', 1, b'regression'), ('patch_radius', 0.1, b'patch radius'),
    ('net_size', 512, b'net size')])
def test_unsupported_configurations_are_refused_with_their_reason(lib, field, value, word):
    from points2surf_amd import weights
    mc = weights.ModelCfg(net_size=1024, points_per_patch=8, sub_sample_size=8, output_dim=2)
    setattr(mc, field, value)
    z = np.zeros(4, np.float32)
    h = ctypes.c_void_p()
    rc = lib.p2s_trainer_create(ctypes.byref(mc), 1, z.ctypes.data_as(ctypes.c_void_p), 4, z.ctypes.data_as(ctypes.c_void_p), 4,
                                0, 0, ctypes.byref(h))
    assert rc == -1 and word in lib.p2s_last_error(), lib.p2s_last_error()


def test_python_refusals_name_the_reason():
    from points2surf_amd import synth, train
    for model, word in (('p2s_vanilla', 'QSTN'), ('p2s_shared_encoder', 'QSTN'), ('p2s_max_sum', 'sum pooling'),
                        ('p2s_regression', 'QSTN'), ('p2s_small_radius', 'QSTN')):
        _, cfg = synth.make_weights(model)
        with pytest.raises(ValueError, match=word):
            train.Trainer(cfg)
    _, cfg = synth.make_weights('p2s_max')
    for change, word in ((dict(output_dim=1), 'regression'), (dict(patch_radius=0.1), 'patch radius'), (dict(net_size=512), 'net size'),
                         (dict(single_transformer=True), 'shared encoder'), (dict(shared_transformer=True), 'shared transformer')):
        with pytest.raises(ValueError, match=word):
            train.Trainer(dict(cfg, **change))


def test_initial_state_has_the_reference_layout():
    from points2surf_amd import model_spec, train
    for stn in (True, False):
        sd = train.init_state(dict(use_feat_stn=stn), seed=5)
        shapes = model_spec.state_shapes(use_feat_stn=stn)
        assert list(sd) == list(shapes)
        for k, v in sd.items():
            assert tuple(v.shape) == tuple(shapes[k]) and v.dtype == (np.int64 if k.endswith('num_batches_tracked') else np.float32), k
        w = sd['fc2.weight']
        assert np.abs(w).max() <= 1 / np.sqrt(1024) and np.abs(w).max() > 0.9 / np.sqrt(1024)      # kaiming_uniform(a = sqrt 5)
        assert np.array_equal(train.init_state(dict(use_feat_stn=stn), seed=5)['fc2.weight'], w)


def test_epoch_order_and_schedule():
    from points2surf_amd import train
    o = train.epoch_order([10, 3], 4, seed=1, epoch=0)
    assert o.shape == (7, 2) and sorted(o[o[:, 0] == 1, 1]) == [0, 1, 2] and len(set(o[o[:, 0] == 0, 1])) == 4
    assert np.array_equal(o, train.epoch_order([10, 3], 4, seed=1, epoch=0))
    assert not np.array_equal(o, train.epoch_order([10, 3], 4, seed=1, epoch=1))
    lrs = [train.learning_rate(0.01, [2, 4], e) for e in range(5)]
    np.testing.assert_allclose(lrs, [0.01, 0.01, 0.001, 0.001, 0.0001], rtol=1e-12)
