"""The cloud-set entry points, p2s_train_losses and the loader / validation options (CPU: symbols, prototypes, refusals that
need no device, argument defaults, the validation order)."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOADER_SYMBOLS = ['p2s_cloudset_create', 'p2s_cloudset_destroy', 'p2s_cloudset_knn_patch', 'p2s_cloudset_size',
                  'p2s_cloudset_subsample_uniform', 'p2s_train_losses']
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    from points2surf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbols_declared_bound_and_exported(lib):
    from points2surf_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'p2s_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(p2s_[a-z0-9_]+)\s*\(', src))
    for s in LOADER_SYMBOLS:
        assert s in declared and s in _lib.PROTOTYPES and hasattr(lib, s), s
        assert not s.startswith('p2s_trainer_')
    assert 'typedef struct p2s_cloudset_s *p2s_cloudset_t;' in src
    assert lib.p2s_abi_version() == 5


def test_create_refuses_null_and_empty(lib):
    h = ctypes.c_void_p()
    one = (ctypes.c_void_p * 1)(None)
    arr = ctypes.cast(one, ctypes.POINTER(ctypes.c_void_p))
    assert lib.p2s_cloudset_create(None, 1, 0, ctypes.byref(h)) == EINVAL and b'p2s_cloudset_create' in lib.p2s_last_error()
    assert lib.p2s_cloudset_create(arr, 0, 0, ctypes.byref(h)) == EINVAL
    assert lib.p2s_cloudset_create(arr, -3, 0, ctypes.byref(h)) == EINVAL
    assert lib.p2s_cloudset_create(arr, 1, 0, None) == EINVAL
    assert lib.p2s_cloudset_create(arr, 1, 0, ctypes.byref(h)) == EINVAL and b'cloud 0 is NULL' in lib.p2s_last_error()
    assert not h.value
    assert lib.p2s_cloudset_destroy(None) == 0
    assert lib.p2s_cloudset_size(None, None, None) == EINVAL


def test_calls_on_a_null_set_are_refused(lib):
    co = np.zeros(2, np.int32)
    p = co.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(64)                                    # never dereferenced: the set is checked first
    assert lib.p2s_cloudset_knn_patch(None, p, fake, 2, 8, None, None, None, None) == EINVAL
    assert b'p2s_cloudset_knn_patch' in lib.p2s_last_error()
    assert lib.p2s_cloudset_subsample_uniform(fake, None, p, 2, 8, None, None, None) == EINVAL
    assert b'p2s_cloudset_subsample_uniform' in lib.p2s_last_error()
    assert lib.p2s_cloudset_subsample_uniform(None, None, p, 2, 8, None, None, None) == EINVAL


@pytest.mark.parametrize('B', [0, -1])
def test_train_losses_refuses_an_empty_batch(lib, B):
    fake = ctypes.c_void_p(64)                                    # never dereferenced: B is checked before any device call
    out = (ctypes.c_double * 2)()
    assert lib.p2s_train_losses(fake, fake, fake, fake, B, out, None) == EINVAL
    assert b'p2s_train_losses' in lib.p2s_last_error() and (b'B = %d' % B) in lib.p2s_last_error()
    assert lib.p2s_train_losses(None, fake, fake, fake, 4, out, None) == EINVAL


def test_argument_defaults_and_saved_parameters():
    from points2surf_amd import train
    base = ['--indir', 'a', '--name', 'b', '--outdir', 'c']
    opt = train.parse_arguments(base)
    assert opt.loader == 'per_shape' and opt.testset == ''
    ns = train.params_namespace(opt)
    assert ns.loader == 'per_shape' and ns.testset == ''
    opt = train.parse_arguments(base + ['--loader', 'set', '--testset', 'testset.txt'])
    ns = train.params_namespace(opt)
    assert (ns.loader, ns.testset) == ('set', 'testset.txt')
    with pytest.raises(SystemExit):
        train.parse_arguments(base + ['--loader', 'other'])


def test_validation_order_is_fixed_and_its_own():
    from points2surf_amd import train
    n, pps, seed = [24, 24, 10], 16, 3
    v = train.epoch_order(n, pps, seed, epoch=-1)
    assert np.array_equal(v, train.epoch_order(n, pps, seed, epoch=-1))
    assert v.shape == (16 + 16 + 10, 2)
    assert not np.array_equal(v, train.epoch_order(n, pps, seed, epoch=0))
    assert np.array_equal(train.epoch_order(n, pps, 0, epoch=-1), train.epoch_order(n, pps, 0, epoch=-1))   # seed + epoch < 0


def test_cloud_of_is_converted_to_int32():
    from points2surf_amd import engine
    for given in ([2, 0, 1], (2, 0, 1), np.array([2, 0, 1], np.int64), np.array([[2, 0, 1]], np.uint8)):
        a = engine._cloud_of(given)
        assert a.dtype == np.int32 and a.flags['C_CONTIGUOUS'] and a.tolist() == [2, 0, 1]
    assert engine._cloud_of([]).shape == (0,)
    with pytest.raises(TypeError):
        engine._cloud_of([0.5, 1.0])
