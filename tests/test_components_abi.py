"""Every argument refusal of p2s_mesh_components, p2s_mesh_submesh and p2s_prepare_clusters happens before the device is
touched: P2S_EINVAL with a message that names the argument, on a machine with no device as well (where a call with good
arguments ends in P2S_ENODEVICE).  The pointers are host addresses that nothing may dereference."""
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


def _refused(lib, rc, word):
    msg = lib.p2s_last_error().decode()
    assert rc == P2S_EINVAL and word in msg, (rc, msg)


def _components(lib, p, **kw):
    a = dict(verts=p, V=3, faces=p, F=1, comp=p, cap=1, counts=p, meas=p, rep=(ctypes.c_int64 * 8)())
    a.update(kw)
    return lib.p2s_mesh_components(a['verts'], a['V'], a['faces'], a['F'], a['comp'], a['cap'], a['counts'], a['meas'], a['rep'], 0, None)


@pytest.mark.parametrize('kw,word', [
    (dict(rep=None), 'report_host'), (dict(V=-1), 'n_verts'), (dict(V=BIG), 'n_verts'), (dict(F=-1), 'n_faces'), (dict(F=BIG), 'n_faces'),
    (dict(verts=None), 'verts_dev'), (dict(faces=None), 'faces_dev'), (dict(comp=None), 'comp_out_dev'), (dict(cap=-1), 'cap_components'),
    (dict(counts=None), 'counts_out_dev'), (dict(meas=None), 'measures_out_dev')])
def test_components_refusals(lib, buf, kw, word):
    _refused(lib, _components(lib, buf[1], **kw), word)


def _submesh(lib, p, **kw):
    a = dict(verts=p, V=3, faces=p, F=1, keep=p, vo=p, cv=3, fo=p, so=p, cf=1, vm=p, rep=(ctypes.c_int64 * 3)())
    a.update(kw)
    return lib.p2s_mesh_submesh(a['verts'], a['V'], a['faces'], a['F'], a['keep'], a['vo'], a['cv'], a['fo'], a['so'], a['cf'], a['vm'],
                                a['rep'], 0, None)


@pytest.mark.parametrize('kw,word', [
    (dict(rep=None), 'report_host'), (dict(V=-1), 'n_verts'), (dict(V=BIG), 'n_verts'), (dict(F=-1), 'n_faces'), (dict(F=BIG), 'n_faces'),
    (dict(verts=None), 'verts_dev'), (dict(faces=None), 'faces_dev'), (dict(keep=None), 'keep_dev'), (dict(cv=-1), 'cap_verts'),
    (dict(cf=-1), 'cap_faces'), (dict(vo=None), 'verts_out_dev'), (dict(fo=None), 'faces_out_dev')])
def test_submesh_refusals(lib, buf, kw, word):
    _refused(lib, _submesh(lib, buf[1], **kw), word)


def _clusters(lib, p, **kw):
    a = dict(pts=p, n=4, radius=1.0, min_points=1, label=p, out=p, ids=p, n_out=ctypes.pointer(ctypes.c_int64(0)), info=(ctypes.c_int64 * 4)())
    a.update(kw)
    return lib.p2s_prepare_clusters(a['pts'], a['n'], ctypes.c_double(a['radius']), a['min_points'], a['label'], a['out'], a['ids'], a['n_out'],
                                    a['info'], 0, None)


@pytest.mark.parametrize('kw,word', [
    (dict(pts=None), 'pts_dev'), (dict(out=None), 'pts_out_dev'), (dict(ids=None), 'ids_out_dev'), (dict(n_out=None), 'n_out_host'),
    (dict(n=-1), 'n ='), (dict(n=BIG), 'n ='), (dict(radius=0.0), 'radius'), (dict(radius=-1.0), 'radius'),
    (dict(radius=float('nan')), 'radius'), (dict(radius=float('inf')), 'radius'), (dict(min_points=0), 'min_points')])
def test_clusters_refusals(lib, buf, kw, word):
    _refused(lib, _clusters(lib, buf[1], **kw), word)


def test_good_arguments_reach_the_device_check(lib, buf):
    import torch
    if torch.cuda.is_available():
        return                                      # with a device the host addresses above must not go further
    for rc in (_components(lib, buf[1]), _submesh(lib, buf[1]), _clusters(lib, buf[1])):
        assert rc == P2S_ENODEVICE and b'device' in lib.p2s_last_error()
    # the optional outputs may be NULL
    assert _submesh(lib, buf[1], so=None, vm=None) == P2S_ENODEVICE
    assert _clusters(lib, buf[1], label=None, info=None) == P2S_ENODEVICE


def test_python_wrappers_check_before_the_device():
    from points2surf_amd import prepare
    for radius, min_points in ((0.0, 1), (-1.0, 1), (float('nan'), 1), (1.0, 0)):
        with pytest.raises(ValueError):
            prepare.remove_small_clusters(np.zeros((3, 3), np.float32), radius, min_points)
