"""Every argument refusal of p2s_mesh_render that needs no device happens before the handle is read or the device touched:
P2S_EINVAL with a message that names the argument, on a machine with no device as well (where a call with good arguments ends
in P2S_ENODEVICE).  The handle and the pointers are host addresses that nothing may dereference."""
import ctypes
import os
import re

import numpy as np
import pytest

P2S_EINVAL, P2S_ENODEVICE = -1, -5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def lib():
    from points2surf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def buf():
    a = np.zeros(4096, np.int64)                     # a zeroed stand-in for the handle: device 0
    return a, ctypes.c_void_p(a.ctypes.data)


def good_params(**kw):
    from points2surf_amd import _lib
    p = _lib.RenderParams()
    p.width, p.height, p.samples, p.projection, p.shading, p.ao_rays = 16, 12, 2, 0, 0, 4
    p.eye, p.right, p.up, p.forward = (ctypes.c_double * 3)(0, 0, 3), (ctypes.c_double * 3)(1, 0, 0), (ctypes.c_double * 3)(0, 1, 0), \
        (ctypes.c_double * 3)(0, 0, -1)
    p.tan_half_w, p.tan_half_h, p.half_w, p.half_h = 0.4, 0.3, 1.0, 1.0
    p.ao_radius, p.ao_bias, p.ambient, p.diffuse = 0.1, 0.001, 0.6, 0.4
    p.base_rgb, p.background_rgb = (ctypes.c_double * 3)(0.8, 0.8, 0.8), (ctypes.c_double * 3)(1, 1, 1)
    for k, x in kw.items():
        setattr(p, k, (ctypes.c_double * 3)(*x) if isinstance(x, tuple) else x)
    return p


def _render(lib, buf, prm='good', **kw):
    p = buf[1]
    a = dict(m=p, rgb=p, dirs=p, vrgb=p, depth=p, face=p, stats=(ctypes.c_int64 * 8)(*([-7] * 8)))
    a.update(kw)
    prm = good_params() if prm == 'good' else prm
    rc = lib.p2s_mesh_render(a['m'], ctypes.byref(prm) if prm is not None else None, a['vrgb'], a['dirs'], a['rgb'], a['depth'], a['face'],
                             a['stats'], None)
    assert (a['stats'] is None or list(a['stats']) == [-7] * 8) and not buf[0].any()               # nothing written
    return rc


S = 2.0 ** -0.5
REFUSALS = [
    (dict(m=None), None, 'handle'), (dict(prm=None), None, 'prm'), (dict(rgb=None), None, 'rgb_out_dev'),
    ({}, dict(width=0), 'width'), ({}, dict(height=0), 'height'), ({}, dict(width=-3), 'width'), ({}, dict(samples=0), 'samples'),
    ({}, dict(samples=5), 'samples'), ({}, dict(ao_rays=-1), 'ao_rays'), ({}, dict(ao_rays=65), 'ao_rays'), (dict(dirs=None), None, 'ao_dirs_dev'),
    ({}, dict(ao_rays=0), 'ao_dirs_dev'), ({}, dict(projection=2), 'projection'), ({}, dict(projection=-1), 'projection'),
    ({}, dict(shading=2), 'shading'), ({}, dict(width=1 << 14, height=1 << 13, samples=2), '2^28'),
    ({}, dict(width=1 << 15, height=1 << 14, samples=1), '2^28'), ({}, dict(eye=(0.0, NAN, 3.0)), 'camera'),
    ({}, dict(forward=(0.0, 0.0, INF)), 'camera'), ({}, dict(right=(-INF, 0.0, 0.0)), 'camera'), ({}, dict(up=(NAN, 1.0, 0.0)), 'camera'),
    ({}, dict(tan_half_w=NAN), 'extent'), ({}, dict(tan_half_h=0.0), 'extent'), ({}, dict(tan_half_w=INF), 'extent'),
    ({}, dict(tan_half_h=-0.3), 'extent'), ({}, dict(projection=1, half_w=NAN), 'extent'), ({}, dict(projection=1, half_h=0.0), 'extent'),
    ({}, dict(ao_radius=NAN), 'ao_radius'), ({}, dict(ao_bias=INF), 'ao_bias'), ({}, dict(ambient=NAN), 'ambient'),
    ({}, dict(diffuse=-INF), 'diffuse'), ({}, dict(base_rgb=(0.5, NAN, 0.5)), 'base_rgb'), ({}, dict(background_rgb=(INF, 1.0, 1.0)), 'background_rgb'),
    ({}, dict(right=(1.0 + 2.0 ** -38, 0.0, 0.0)), 'orthonormal'), ({}, dict(up=(2.0 ** -39, 1.0, 0.0)), 'orthonormal'),
    ({}, dict(forward=(0.0, 2.0 ** -39, -1.0)), 'orthonormal'), ({}, dict(right=(0.0, 0.0, 0.0)), 'orthonormal'),
    ({}, dict(right=(S, S, 0.0), up=(S, S, 0.0)), 'orthonormal'), ({}, dict(ao_radius=-1e-9), 'ao_radius'), ({}, dict(ao_bias=-1e-9), 'ao_bias'),
]


@pytest.mark.parametrize('kw,prm,word', REFUSALS)
def test_render_refusals(lib, buf, kw, prm, word):
    kw = dict(kw)
    if 'prm' not in kw and prm is not None:
        kw['prm'] = good_params(**prm)
    rc = _render(lib, buf, **kw)
    msg = lib.p2s_last_error().decode()
    assert rc == P2S_EINVAL and word in msg and 'p2s_mesh_render' in msg, (rc, msg)


def test_the_order_of_the_refusals(lib, buf):
    """the first that applies, in the order of the header"""
    for prm, word in ((dict(width=0, samples=9, ao_rays=99), 'width'), (dict(samples=9, ao_rays=99, eye=(NAN, 0.0, 0.0)), 'samples'),
                      (dict(ao_rays=99, ao_radius=-1.0), 'ao_rays outside'), (dict(eye=(NAN, 0.0, 0.0), right=(0.0, 0.0, 0.0)), 'camera'),
                      (dict(ambient=NAN, right=(0.0, 0.0, 0.0)), 'ambient'), (dict(right=(0.0, 0.0, 0.0), ao_radius=-1.0), 'orthonormal'),
                      (dict(ao_radius=-1.0, ao_bias=-1.0), 'ao_radius < 0')):
        assert _render(lib, buf, prm=good_params(**prm)) == P2S_EINVAL
        assert word in lib.p2s_last_error().decode(), (word, lib.p2s_last_error())
    assert _render(lib, buf, m=None, prm=None, rgb=None) == P2S_EINVAL and b'handle' in lib.p2s_last_error()


def test_good_arguments_reach_the_device_check(lib, buf):
    import torch
    if torch.cuda.is_available():
        return                                      # with a device the host addresses above must not go further
    for prm in (dict(), dict(projection=1), dict(shading=1), dict(samples=4, ao_rays=64), dict(width=1 << 14, height=1 << 14, samples=1),
                dict(ao_radius=0.0, ao_bias=0.0), dict(tan_half_w=1e-9), dict(projection=1, tan_half_w=NAN, tan_half_h=-1.0),
                dict(half_w=NAN, half_h=-1.0), dict(right=(1.0 + 2.0 ** -42, 0.0, 0.0)), dict(ambient=-5.0, diffuse=70.0),
                dict(base_rgb=(-1.0, 2.0, 0.5))):
        assert _render(lib, buf, prm=good_params(**prm)) == P2S_ENODEVICE and b'device' in lib.p2s_last_error()
    assert _render(lib, buf, prm=good_params(ao_rays=0), dirs=None, vrgb=None, depth=None, face=None, stats=None) == P2S_ENODEVICE


def test_the_header_declares_it_and_the_table_binds_it(lib):
    from points2surf_amd import _lib
    text = open(os.path.join(REPO, 'include', 'p2s_hip.h')).read()
    assert re.search(r'\bint p2s_mesh_render\(p2s_trimesh_t m, const p2s_render_params \*prm, const float \*vertex_rgb_dev, '
                     r'const double \*ao_dirs_dev,\s+uint8_t \*rgb_out_dev, double \*depth_out_dev, int32_t \*face_out_dev, '
                     r'int64_t \*stats_host, void \*stream\);', text)
    assert re.search(r'#define P2S_ABI_VERSION 5\b', text) and lib.p2s_abi_version() == 5
    res, args = _lib.PROTOTYPES['p2s_mesh_render']
    assert res is ctypes.c_int and len(args) == 9 and args[7] == ctypes.POINTER(ctypes.c_int64)
    assert lib.p2s_mesh_render.argtypes == args
    body = re.search(r'typedef struct \{([^}]*)\} p2s_render_params;', text).group(1)
    declared = re.findall(r'\b([a-z_]+)(?:\[3\])?\s*[,;]', re.sub(r'/\*.*?\*/', '', body))
    assert declared == [n for n, _ in _lib.RenderParams._fields_]
    assert ctypes.sizeof(_lib.RenderParams) == 6 * 4 + 8 * (12 + 8 + 6)      # no padding: six int32, then 26 doubles
