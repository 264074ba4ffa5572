"""The training test hooks p2s_debug_train_linear / p2s_debug_train_bn / p2s_debug_train_relu_masks (CPU: declared,
bound, exported, and the refusals that are decided before any device call).  What they compute is checked in
tests/test_gpu_train_kernels.py; the masks are used and checked in tests/test_gpu_train.py."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ['p2s_debug_train_bn', 'p2s_debug_train_linear', 'p2s_debug_train_relu_masks']
EINVAL, ECAPACITY = -1, -4


@pytest.fixture(scope='module')
def lib():
    from points2surf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_hooks_declared_bound_and_exported(lib):
    from points2surf_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'p2s_hip.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(p2s_debug_train_[a-z0-9_]+)\s*\(', src))) == HOOKS
    for s in HOOKS:
        assert s in _lib.PROTOTYPES and hasattr(lib, s), s
    assert lib.p2s_abi_version() == 5


def test_training_does_not_use_the_hooks():
    assert 'p2s_debug' not in open(os.path.join(REPO, 'points2surf_amd', 'train.py')).read()


@pytest.mark.parametrize('M,N,K,accum,boff', [(0, 4, 4, 0, 16), (4, 0, 4, 0, 16), (4, 4, 0, 0, 16), (-3, 4, 4, 0, 16), (4, 4, 4, 2, 16),
                                               (4, 4, 4, -1, 16), (4, 4, 4, 0, 15)])
def test_linear_hook_refuses_bad_arguments(lib, M, N, K, accum, boff):
    fake = ctypes.c_void_p(64)                                    # never dereferenced: the sizes are checked first
    assert lib.p2s_debug_train_linear(fake, fake, boff, fake, fake, fake, fake, M, N, K, accum, None) == EINVAL
    assert b'p2s_debug_train_linear' in lib.p2s_last_error() and (b'M = %d' % M) in lib.p2s_last_error()


@pytest.mark.parametrize('M,C,off', [(1, 4, 4), (0, 4, 4), (4, 0, 4), (4, -2, 4), (4, 4, 3)])
def test_bn_hook_refuses_bad_arguments(lib, M, C, off):
    fake = ctypes.c_void_p(64)
    assert lib.p2s_debug_train_bn(fake, fake, off, fake, fake, fake, fake, fake, fake, M, C, 0, None) == EINVAL
    assert b'p2s_debug_train_bn' in lib.p2s_last_error() and (b'M = %d' % M) in lib.p2s_last_error()


def test_hooks_refuse_more_than_2_31_values(lib):
    fake = ctypes.c_void_p(64)
    assert lib.p2s_debug_train_linear(fake, fake, 8, fake, fake, fake, fake, 1 << 30, 4, 2, 0, None) == ECAPACITY
    assert lib.p2s_debug_train_bn(fake, fake, 4, fake, fake, fake, fake, fake, fake, 1 << 30, 4, 0, None) == ECAPACITY
    assert b'2^31' in lib.p2s_last_error()


def test_relu_mask_hook_refuses_null(lib):
    out = (ctypes.c_uint8 * 4)()
    assert lib.p2s_debug_train_relu_masks(None, out, 4) == EINVAL and b'p2s_debug_train_relu_masks' in lib.p2s_last_error()
