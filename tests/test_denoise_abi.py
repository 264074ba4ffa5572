"""Every argument refusal of p2s_mesh_denoise happens before the device is touched: P2S_EINVAL with a message that names the
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


def _denoise(lib, buf, **kw):
    p, q = buf[2], buf[3]
    a = dict(verts=p, V=3, faces=p, F=1, T=0.5, nit=10, vit=10, mode=0, fixed=p, out=q, nrm=p, cls=p, rep=(ctypes.c_int64 * 16)())
    a.update(kw)
    return lib.p2s_mesh_denoise(a['verts'], a['V'], a['faces'], a['F'], a['T'], a['nit'], a['vit'], a['mode'], a['fixed'], a['out'], a['nrm'],
                                a['cls'], a['rep'], 0, None)


@pytest.mark.parametrize('kw,word', [
    (dict(rep=None), 'report_host'), (dict(V=-1), 'n_verts'), (dict(V=BIG), 'n_verts'), (dict(F=-1), 'n_faces'), (dict(F=BIG), 'n_faces'),
    (dict(verts=None), 'verts_dev'), (dict(faces=None), 'faces_dev'), (dict(T=1.0), 'threshold'), (dict(T=-1e-9), 'threshold'),
    (dict(T=1.5), 'threshold'), (dict(T=float('nan')), 'threshold'), (dict(T=float('inf')), 'threshold'),
    (dict(T=float('-inf')), 'threshold'), (dict(nit=-1), 'normal_iterations'), (dict(nit=10001), 'normal_iterations'),
    (dict(vit=-1), 'vertex_iterations'), (dict(vit=10001), 'vertex_iterations'), (dict(mode=-1), 'boundary_mode'),
    (dict(mode=2), 'boundary_mode'), (dict(out=None), 'verts_out_dev'), (dict(out='same'), 'verts_out_dev'),
    (dict(out='inside'), 'verts_out_dev')])
def test_denoise_refusals(lib, buf, kw, word):
    if kw.get('out') == 'same':
        kw = dict(out=buf[2])
    elif kw.get('out') == 'inside':
        kw = dict(out=ctypes.c_void_p(buf[0].ctypes.data + 12))         # overlaps the 36 bytes of the three input vertices
    rc = _denoise(lib, buf, **kw)
    msg = lib.p2s_last_error().decode()
    assert rc == P2S_EINVAL and word in msg and 'p2s_mesh_denoise' in msg, (rc, msg)


def test_good_arguments_reach_the_device_check(lib, buf):
    import torch
    if torch.cuda.is_available():
        return                                      # with a device the host addresses above must not go further
    for kw in (dict(), dict(T=0.0), dict(T=-0.0), dict(T=0.9999999), dict(nit=0, vit=0), dict(nit=10000, vit=10000), dict(mode=1)):
        assert _denoise(lib, buf, **kw) == P2S_ENODEVICE and b'device' in lib.p2s_last_error()
    assert _denoise(lib, buf, fixed=None, nrm=None, cls=None) == P2S_ENODEVICE         # the mask and two of the outputs may be NULL
    assert _denoise(lib, buf, faces=None, F=0) == P2S_ENODEVICE
    assert _denoise(lib, buf, verts=None, V=0, faces=None, F=0, out=None) == P2S_ENODEVICE


def test_the_header_declares_it_and_the_table_binds_it(lib):
    from points2surf_amd import _lib
    text = open(os.path.join(REPO, 'include', 'p2s_hip.h')).read()
    assert re.search(r'\bint p2s_mesh_denoise\(const float \*verts_dev, int64_t n_verts, const int32_t \*faces_dev, int64_t n_faces, '
                     r'double threshold,\s+int normal_iterations, int vertex_iterations, int boundary_mode, const uint8_t \*fixed_dev, '
                     r'float \*verts_out_dev,\s+float \*normals_out_dev, uint8_t \*class_out_dev, int64_t \*report_host, int device, '
                     r'void \*stream\);', text)
    res, args = _lib.PROTOTYPES['p2s_mesh_denoise']
    assert res is ctypes.c_int and len(args) == 15 and args[4] is ctypes.c_double
    assert [a for a in args[5:8]] == [ctypes.c_int] * 3 and args[12] == ctypes.POINTER(ctypes.c_int64)
    assert lib.p2s_mesh_denoise.argtypes == args


def test_the_python_wrappers_check_before_the_device():
    from points2surf_amd import denoise
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    for kw in (dict(threshold=1.0), dict(threshold=-0.1), dict(threshold=float('nan')), dict(threshold=float('inf')),
               dict(normal_iterations=-1), dict(normal_iterations=10001), dict(normal_iterations=2.5), dict(normal_iterations=True),
               dict(vertex_iterations=-1), dict(vertex_iterations=10001), dict(vertex_iterations=0.5), dict(vertex_iterations=False),
               dict(boundary='curve'), dict(boundary=1)):
        with pytest.raises(ValueError):
            denoise.denoise(v, f, **kw)
        with pytest.raises(ValueError):
            denoise.denoise_dir('nowhere', 'nowhere', **kw)
        with pytest.raises(ValueError):
            denoise.denoise_file('nowhere.ply', 'nowhere.ply', **kw)
    bits = int(np.array([2.25], np.float64).view(np.int64)[0])
    assert denoise.report_dict([9 | (7 << 32), 4, 1, 2, 1, 1, 3, 12, 10, 5, bits, 0, 0, 0, 0, 0]) == dict(
        verts_in=9, faces_in=7, free=4, boundary_fixed=1, masked=2, unreferenced=1, no_live_face=1, dead_faces=3, max_neighbours=12,
        normal_iterations_run=10, vertex_iterations_run=5, max_displacement=1.5, nonfinite=0)
    assert tuple(denoise.report_dict([0] * 16)) == denoise.REPORT_KEYS
    assert len(denoise.CLASSES) == 5 and denoise.REPORT_COLUMNS[-1] == 'verdict'
