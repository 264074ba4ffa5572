"""Every argument refusal of p2s_mesh_smooth happens before the device is touched: P2S_EINVAL with a message that names the
argument, on a machine with no device as well (where a call with good arguments ends in P2S_ENODEVICE).  The pointers are
host addresses that nothing may dereference."""
import ctypes
import os
import re

import numpy as np
import pytest

P2S_EINVAL, P2S_ENODEVICE = -1, -5
BIG = (1 << 27) + 1
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from points2surf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def buf():
    a, b = np.zeros(64, np.int64), np.zeros(64, np.int64)
    return a, b, ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(b.ctypes.data)


def _smooth(lib, buf, **kw):
    p, q = buf[2], buf[3]
    a = dict(verts=p, V=3, faces=p, F=1, it=10, lam=0.5, mu=-0.53, mode=0, fixed=p, out=q, cls=p, rep=(ctypes.c_int64 * 16)())
    a.update(kw)
    return lib.p2s_mesh_smooth(a['verts'], a['V'], a['faces'], a['F'], a['it'], a['lam'], a['mu'], a['mode'], a['fixed'], a['out'], a['cls'],
                               a['rep'], 0, None)


@pytest.mark.parametrize('kw,word', [
    (dict(rep=None), 'report_host'), (dict(V=-1), 'n_verts'), (dict(V=BIG), 'n_verts'), (dict(F=-1), 'n_faces'), (dict(F=BIG), 'n_faces'),
    (dict(verts=None), 'verts_dev'), (dict(faces=None), 'faces_dev'), (dict(it=-1), 'iterations'), (dict(it=10001), 'iterations'),
    (dict(lam=0.0), 'lambda'), (dict(lam=-0.5), 'lambda'), (dict(lam=1.0000001), 'lambda'), (dict(lam=float('nan')), 'lambda'),
    (dict(lam=float('inf')), 'lambda'), (dict(mu=0.1), 'mu'), (dict(mu=-2.0000001), 'mu'), (dict(mu=float('nan')), 'mu'),
    (dict(mu=float('-inf')), 'mu'), (dict(mode=-1), 'boundary_mode'), (dict(mode=3), 'boundary_mode'), (dict(out=None), 'verts_out_dev'),
    (dict(out='same'), 'verts_out_dev'), (dict(out='inside'), 'verts_out_dev')])
def test_smooth_refusals(lib, buf, kw, word):
    if kw.get('out') == 'same':
        kw = dict(out=buf[2])
    elif kw.get('out') == 'inside':
        kw = dict(out=ctypes.c_void_p(buf[0].ctypes.data + 12))         # overlaps the 36 bytes of the three input vertices
    rc = _smooth(lib, buf, **kw)
    msg = lib.p2s_last_error().decode()
    assert rc == P2S_EINVAL and word in msg and 'p2s_mesh_smooth' in msg, (rc, msg)


def test_good_arguments_reach_the_device_check(lib, buf):
    import torch
    if torch.cuda.is_available():
        return                                      # with a device the host addresses above must not go further
    for kw in (dict(), dict(it=0), dict(it=10000), dict(lam=1.0, mu=-2.0), dict(mu=0.0), dict(mu=-0.0), dict(mode=1), dict(mode=2)):
        assert _smooth(lib, buf, **kw) == P2S_ENODEVICE and b'device' in lib.p2s_last_error()
    assert _smooth(lib, buf, fixed=None, cls=None) == P2S_ENODEVICE     # the mask and the classes may be NULL
    assert _smooth(lib, buf, faces=None, F=0) == P2S_ENODEVICE
    assert _smooth(lib, buf, verts=None, V=0, faces=None, F=0, out=None) == P2S_ENODEVICE


def test_the_header_declares_it_and_the_table_binds_it(lib):
    from points2surf_amd import _lib
    text = open(os.path.join(REPO, 'include', 'p2s_hip.h')).read()
    assert re.search(r'\bint p2s_mesh_smooth\(const float \*verts_dev, int64_t n_verts, const int32_t \*faces_dev, int64_t n_faces, '
                     r'int iterations, double lambda,\s+double mu, int boundary_mode, const uint8_t \*fixed_dev, float \*verts_out_dev, '
                     r'uint8_t \*class_out_dev,\s+int64_t \*report_host, int device, void \*stream\);', text)
    res, args = _lib.PROTOTYPES['p2s_mesh_smooth']
    assert res is ctypes.c_int and len(args) == 14 and args[5] is ctypes.c_double and args[6] is ctypes.c_double
    assert lib.p2s_mesh_smooth.argtypes == args and lib.p2s_abi_version() == 5


def test_the_python_wrappers_check_before_the_device():
    from points2surf_amd import smooth
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    for kw in (dict(iterations=-1), dict(iterations=10001), dict(iterations=2.5), dict(iterations=True), dict(lam=0.0), dict(lam=1.5),
               dict(lam=float('nan')), dict(mu=0.5), dict(mu=-2.5), dict(mu=float('nan')), dict(boundary='open'), dict(boundary=1)):
        with pytest.raises(ValueError):
            smooth.smooth(v, f, **kw)
        with pytest.raises(ValueError):
            smooth.smooth_dir('nowhere', 'nowhere', **kw)
        with pytest.raises(ValueError):
            smooth.smooth_file('nowhere.ply', 'nowhere.ply', **kw)
    bits = int(np.array([2.25], np.float64).view(np.int64)[0])
    assert smooth.report_dict([9 | (7 << 32), 4, 1, 2, 0, 1, 1, 15, 6, 20, bits, 0, 0, 0, 0, 0]) == dict(
        verts_in=9, faces_in=7, free=4, boundary_curve=1, boundary_fixed=2, nonmanifold_fixed=0, masked=1, unreferenced=1, edges=15,
        max_neighbours=6, half_steps=20, max_displacement=1.5, nonfinite=0)
    assert tuple(smooth.report_dict([0] * 16)) == smooth.REPORT_KEYS
