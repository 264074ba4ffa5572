"""Every argument refusal of p2s_mesh_manifold happens before the device is touched: P2S_EINVAL with a message that names the
argument, on a machine with no device as well (where a call with good arguments ends in P2S_ENODEVICE).  The pointers are
host addresses that nothing may dereference."""
import ctypes

import numpy as np
import pytest

P2S_EINVAL, P2S_ENODEVICE = -1, -5
BIG = (1 << 27) + 1


@pytest.fixture(scope='module')
def lib():
    from points2surf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def buf():
    a = np.zeros(64, np.int64)
    return a, ctypes.c_void_p(a.ctypes.data)


def _manifold(lib, p, **kw):
    a = dict(verts=p, V=3, faces=p, F=1, mode=2, vo=p, cv=3, fo=p, cf=1, vs=p, fs=p, rep=(ctypes.c_int64 * 16)())
    a.update(kw)
    return lib.p2s_mesh_manifold(a['verts'], a['V'], a['faces'], a['F'], a['mode'], a['vo'], a['cv'], a['fo'], a['cf'], a['vs'], a['fs'],
                                 a['rep'], 0, None)


@pytest.mark.parametrize('kw,word', [
    (dict(rep=None), 'report_host'), (dict(V=-1), 'n_verts'), (dict(V=BIG), 'n_verts'), (dict(F=-1), 'n_faces'), (dict(F=BIG), 'n_faces'),
    (dict(verts=None), 'verts_dev'), (dict(faces=None), 'faces_dev'), (dict(mode=0), 'mode'), (dict(mode=4), 'mode'), (dict(mode=-1), 'mode'),
    (dict(cv=-1), 'cap_verts'), (dict(cf=-1), 'cap_faces'), (dict(vo=None), 'verts_out_dev'), (dict(fo=None), 'faces_out_dev')])
def test_manifold_refusals(lib, buf, kw, word):
    rc = _manifold(lib, buf[1], **kw)
    msg = lib.p2s_last_error().decode()
    assert rc == P2S_EINVAL and word in msg and 'p2s_mesh_manifold' in msg, (rc, msg)


def test_good_arguments_reach_the_device_check(lib, buf):
    import torch
    if torch.cuda.is_available():
        return                                      # with a device the host addresses above must not go further
    for mode in (1, 2, 3):
        assert _manifold(lib, buf[1], mode=mode) == P2S_ENODEVICE and b'device' in lib.p2s_last_error()
    # the optional outputs may be NULL; so may the buffers of a capacity 0
    assert _manifold(lib, buf[1], vs=None, fs=None) == P2S_ENODEVICE
    assert _manifold(lib, buf[1], vo=None, cv=0, fo=None, cf=0) == P2S_ENODEVICE
    assert _manifold(lib, buf[1], verts=None, V=0, faces=None, F=0) == P2S_ENODEVICE


def test_the_python_wrapper_checks_before_the_device():
    from points2surf_amd import manifold
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    with pytest.raises(ValueError):
        manifold.manifold(v, f, edges='both')
    with pytest.raises(ValueError):
        manifold.manifold(v, f, edges='split', split=False)
    with pytest.raises(ValueError):
        manifold.remove_fill_split(v, f, max_hole_edges=65)
    with pytest.raises(ValueError):
        manifold.manifold_dir('nowhere', 'nowhere', edges='both')
    with pytest.raises(ValueError):
        manifold.manifold(v[:, :2], f)
    assert manifold.report_dict([3 | (1 << 32), 3, 1, 0, 0, 0, 0, 0, 3, 3, 0, 1, 0, 0, 0, 0]) == dict(
        verts_in=3, faces_in=1, verts_out=3, faces_out=1, nonmanifold_edges_in=0, faces_removed=0, vertices_split=0, vertices_added=0,
        vertices_dropped=0, boundary_edges_in=3, boundary_edges_out=3, rejoined_edges=0, hook_rounds=1)
