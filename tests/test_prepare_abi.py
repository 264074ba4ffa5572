"""The p2s_prepare_* entry points are exported, have ctypes prototypes and refuse bad arguments by name before they touch a
device (no compute)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('p2s_prepare_finite', 'p2s_prepare_crop', 'p2s_prepare_outliers', 'p2s_prepare_voxel_thin', 'p2s_prepare_normalize',
           'p2s_prepare_gather', 'p2s_prepare_restore')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    from points2surf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbols_exported_declared_and_documented(lib):
    from points2surf_amd import _lib
    header = open(os.path.join(REPO, 'include', 'p2s_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    doc = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.PROTOTYPES and getattr(lib, s).argtypes == _lib.PROTOTYPES[s][1], s
        assert re.search(r'\b%s\s*\(' % s, header), s
        assert '`%s(' % s in doc, s
    assert lib.p2s_abi_version() == 5


def _refused(lib, rc, word):
    msg = lib.p2s_last_error().decode()
    assert rc == EINVAL, (rc, msg)
    assert word in msg, msg


def test_bad_arguments_are_refused_by_name(lib):
    buf = (ctypes.c_float * 64)()                    # never read: every call below is refused before the device is touched
    p = ctypes.cast(buf, ctypes.c_void_p)
    m = ctypes.c_int64(0)
    pm = ctypes.byref(m)
    centre = (ctypes.c_double * 3)()
    # null pointers
    _refused(lib, lib.p2s_prepare_finite(None, 4, p, p, pm, 0, None), 'pts_dev')
    _refused(lib, lib.p2s_prepare_finite(p, 4, None, p, pm, 0, None), 'pts_out_dev')
    _refused(lib, lib.p2s_prepare_finite(p, 4, p, None, pm, 0, None), 'ids_out_dev')
    _refused(lib, lib.p2s_prepare_finite(p, 4, p, p, None, 0, None), 'n_out_host')
    _refused(lib, lib.p2s_prepare_crop(None, 4, 0.01, 1.0, p, p, pm, None, 0, None), 'pts_dev')
    _refused(lib, lib.p2s_prepare_outliers(p, 4, 2, 2.0, None, None, p, pm, None, 0, None), 'pts_out_dev')
    _refused(lib, lib.p2s_prepare_voxel_thin(p, 4, 2, 0, p, None, pm, None, 0, None), 'ids_out_dev')
    _refused(lib, lib.p2s_prepare_normalize(None, 4, p, None, 0, None), 'pts_dev')
    _refused(lib, lib.p2s_prepare_normalize(p, 4, None, None, 0, None), 'pts_out_dev')
    _refused(lib, lib.p2s_prepare_gather(p, 4, 3, None, 2, p, 0, None), 'ids_dev')
    _refused(lib, lib.p2s_prepare_restore(p, 4, None, 1.0, p, 0, None), 'centre_host')
    # counts
    _refused(lib, lib.p2s_prepare_finite(p, -1, p, p, pm, 0, None), 'n = -1')
    _refused(lib, lib.p2s_prepare_normalize(p, 0, p, None, 0, None), 'n = 0')
    # k
    for k in (0, -3, 65):
        _refused(lib, lib.p2s_prepare_outliers(p, 4, k, 2.0, None, p, p, pm, None, 0, None), 'k = %d' % k)
    # std_ratio
    _refused(lib, lib.p2s_prepare_outliers(p, 4, 2, -0.5, None, p, p, pm, None, 0, None), 'std_ratio')
    _refused(lib, lib.p2s_prepare_outliers(p, 4, 2, float('nan'), None, p, p, pm, None, 0, None), 'std_ratio')
    # quantile outside [0, 0.5), margin
    for q in (-0.01, 0.5, 0.75, float('nan')):
        _refused(lib, lib.p2s_prepare_crop(p, 4, q, 1.0, p, p, pm, None, 0, None), 'quantile')
    _refused(lib, lib.p2s_prepare_crop(p, 4, 0.01, -1.0, p, p, pm, None, 0, None), 'margin')
    # resolution outside 1 .. 1024 (0 asks for the search, which needs a budget)
    for r in (-1, 1025):
        _refused(lib, lib.p2s_prepare_voxel_thin(p, 4, 2, r, p, p, pm, None, 0, None), 'resolution = %d' % r)
    _refused(lib, lib.p2s_prepare_voxel_thin(p, 4, 0, 0, p, p, pm, None, 0, None), 'resolution')
    # gather, restore
    _refused(lib, lib.p2s_prepare_gather(p, 4, 0, p, 2, p, 0, None), 'width')
    _refused(lib, lib.p2s_prepare_restore(p, 4, centre, 0.0, p, 0, None), 'scale')
    assert m.value == 0


def test_python_layer_refuses_before_the_library():
    from points2surf_amd import prepare
    import numpy as np
    with pytest.raises(ValueError, match='resolution'):
        prepare.voxel_thin(np.zeros((4, 3), np.float32), 2, resolution=0)
    with pytest.raises(ValueError, match='max_points'):
        prepare.voxel_thin(np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError, match='unknown options'):
        prepare.prepare(np.zeros((4, 3), np.float32), crop=0.1)
    with pytest.raises(ValueError, match='thin'):
        prepare.prepare(np.zeros((4, 3), np.float32), thin='grid')
