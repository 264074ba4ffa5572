"""p2s_mesh_simplify is exported, has its ctypes prototype, is declared and documented, and refuses bad arguments by name
before it touches a device (no compute)."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = 'p2s_mesh_simplify'
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    from points2surf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbol_exported_bound_declared_and_documented(lib):
    from points2surf_amd import _lib
    header = open(os.path.join(REPO, 'include', 'p2s_hip.h')).read()
    assert re.search(r'#define\s+P2S_ABI_VERSION\s+5\b', header)
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    doc = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    assert hasattr(lib, SYMBOL)
    assert SYMBOL in _lib.PROTOTYPES and getattr(lib, SYMBOL).argtypes == _lib.PROTOTYPES[SYMBOL][1]
    assert len(_lib.PROTOTYPES[SYMBOL][1]) == 17
    assert re.search(r'\b%s\s*\(' % SYMBOL, header)
    assert '`%s(' % SYMBOL in doc
    assert lib.p2s_abi_version() == 5


def _call(lib, **kw):
    """one valid call with the named arguments replaced; never reaches a device when an argument is bad"""
    buf = (ctypes.c_float * 64)()                    # never read
    p = ctypes.cast(buf, ctypes.c_void_p)
    rep = (ctypes.c_int64 * 16)(*([-7] * 16))
    a = dict(verts_dev=p, n_verts=4, faces_dev=p, n_faces=2, resolution=8, max_faces=1, placement=1, epsilon=1e-3,
             verts_out_dev=p, cap_verts=4, faces_out_dev=p, face_src_out_dev=p, cap_faces=2, vert_map_out_dev=p,
             report_host=rep, device=0, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = lib.p2s_mesh_simplify(a['verts_dev'], a['n_verts'], a['faces_dev'], a['n_faces'], a['resolution'], a['max_faces'],
                               a['placement'], ctypes.c_double(a['epsilon']), a['verts_out_dev'], a['cap_verts'],
                               a['faces_out_dev'], a['face_src_out_dev'], a['cap_faces'], a['vert_map_out_dev'], a['report_host'],
                               a['device'], a['stream'])
    return rc, lib.p2s_last_error().decode(), list(rep)


def _refused(lib, word, **kw):
    rc, msg, rep = _call(lib, **kw)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith('p2s_mesh_simplify: bad argument') and word in msg, msg
    assert rep == [-7] * 16                          # nothing was written


def test_bad_arguments_are_refused_by_name(lib):
    for name in ('verts_dev', 'faces_dev', 'verts_out_dev', 'faces_out_dev', 'report_host'):
        _refused(lib, name, **{name: None})
    for r in (-1, 1025, 1 << 20):
        _refused(lib, 'resolution', resolution=r)
    _refused(lib, 'max_faces', resolution=0, max_faces=-1)
    for pl in (-1, 2, 7):
        _refused(lib, 'placement', placement=pl)
    for e in (float('nan'), float('inf'), -float('inf'), 0.0, 0.99e-6, 1.0000001, -1e-3):
        _refused(lib, 'epsilon', epsilon=e)
    for name in ('n_verts', 'n_faces', 'cap_verts', 'cap_faces'):
        _refused(lib, name, **{name: -1})
    for name in ('n_verts', 'n_faces'):
        _refused(lib, name, **{name: (1 << 27) + 1})


def test_no_device_is_a_loud_error(lib):
    """valid arguments and a device that does not exist: an error code, no crash, nothing read"""
    rc, msg, _ = _call(lib, device=1 << 20)
    assert rc == -5 and 'device' in msg, (rc, msg)


def test_python_layer_refuses_before_the_library():
    from points2surf_amd import simplify
    v, f = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    with pytest.raises(ValueError, match='placement'):
        simplify.simplify(v, f, placement='median')
    with pytest.raises(ValueError, match='resolution'):
        simplify.simplify(v, f, resolution=1025)
    with pytest.raises(ValueError, match='max_faces'):
        simplify.simplify(v, f, max_faces=-1)
    with pytest.raises(ValueError, match='max_faces'):
        simplify.simplify(v, f, max_faces=None)
    for e in (0.0, 2.0, float('nan')):
        with pytest.raises(ValueError, match='epsilon'):
            simplify.simplify(v, f, epsilon=e)
    with pytest.raises(SystemExit):
        simplify.main(['--indir', 'a', '--outdir', 'b', '--placement', 'median'])
    assert simplify.report_dict([3 | (5 << 32), 1, 2, 9, 4, 5, 6, 7, 8, 9, 10, 11, 2 | (1 << 32), 0, 0, 0]) == dict(
        verts_in=3, faces_in=5, verts_out=1, faces_out=2, resolution=9, cells_occupied=4, faces_collapsed=5, faces_duplicate=6,
        faces_degenerate=7, cells_quadric=8, cells_trace_zero=9, cells_fallback=10, probes=11, boundary_edges_out=2,
        nonmanifold_edges_out=1, boundary_edges_in=0, nonmanifold_edges_in=0)
    assert set(simplify.REPORT_KEYS) == set(simplify.report_dict([0] * 16))
