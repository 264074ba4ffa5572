"""Every argument refusal of p2s_mesh_fill_holes happens before the device is touched: P2S_EINVAL with a message that names the
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


def _fill(lib, p, **kw):
    a = dict(verts=p, V=3, faces=p, F=1, K=30, fo=p, cf=4, fs=p, ho=p, ha=p, ch=1, rep=(ctypes.c_int64 * 16)())
    a.update(kw)
    return lib.p2s_mesh_fill_holes(a['verts'], a['V'], a['faces'], a['F'], a['K'], a['fo'], a['cf'], a['fs'], a['ho'], a['ha'], a['ch'],
                                   a['rep'], 0, None)


@pytest.mark.parametrize('kw,word', [
    (dict(rep=None), 'report_host'), (dict(V=-1), 'n_verts'), (dict(V=BIG), 'n_verts'), (dict(F=-1), 'n_faces'), (dict(F=BIG), 'n_faces'),
    (dict(verts=None), 'verts_dev'), (dict(faces=None), 'faces_dev'), (dict(K=-1), 'max_hole_edges'), (dict(K=129), 'max_hole_edges'),
    (dict(cf=-1), 'cap_faces'), (dict(ch=-1), 'cap_holes'), (dict(fo=None), 'faces_out_dev')])
def test_fill_holes_refusals(lib, buf, kw, word):
    rc = _fill(lib, buf[1], **kw)
    msg = lib.p2s_last_error().decode()
    assert rc == P2S_EINVAL and word in msg and 'p2s_mesh_fill_holes' in msg, (rc, msg)


def test_good_arguments_reach_the_device_check(lib, buf):
    import torch
    if torch.cuda.is_available():
        return                                      # with a device the host addresses above must not go further
    for K in (0, 30, 128):
        assert _fill(lib, buf[1], K=K) == P2S_ENODEVICE and b'device' in lib.p2s_last_error()
    # the optional outputs may be NULL; so may the buffer of a capacity 0
    assert _fill(lib, buf[1], fs=None, ho=None, ha=None, ch=0) == P2S_ENODEVICE
    assert _fill(lib, buf[1], fo=None, cf=0) == P2S_ENODEVICE
    assert _fill(lib, buf[1], verts=None, V=0, faces=None, F=0) == P2S_ENODEVICE


def test_the_python_wrappers_check_before_the_device():
    from points2surf_amd import holes, manifold
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    for bad in (-1, 129, 2.5, True):
        with pytest.raises(ValueError):
            holes.fill(v, f, max_hole_edges=bad)
    with pytest.raises(ValueError):
        holes.fill(v[:, :2], f)
    with pytest.raises(ValueError):
        holes.fill(v, f.reshape(-1))
    with pytest.raises(ValueError):
        holes.fill_dir('nowhere', 'nowhere', max_hole_edges=200)
    with pytest.raises(ValueError):
        holes.fill_file('nowhere.ply', 'nowhere.ply', max_hole_edges=-3)
    # the opt-in of manifold: the default keeps the fan and its bound; 'area' has the bound of the new unit
    with pytest.raises(ValueError):
        manifold.remove_fill_split(v, f, max_hole_edges=65)
    with pytest.raises(ValueError):
        manifold.remove_fill_split(v, f, max_hole_edges=65, fill='fan')
    with pytest.raises(ValueError):
        manifold.remove_fill_split(v, f, max_hole_edges=129, fill='area')
    with pytest.raises(ValueError):
        manifold.remove_fill_split(v, f, fill='ears')
    with pytest.raises(ValueError):
        manifold.manifold_dir('nowhere', 'nowhere', edges='remove', max_hole_edges=129, fill='area')
    assert holes.report_dict([9 | (7 << 32), 10, 2, 1, 3, 1, 0, 12, 7, 1, 5, 0, 0, 0, 0, 0]) == dict(
        verts_in=9, faces_in=7, faces_out=10, loops_found=2, holes_filled=1, faces_added=3, loops_too_long=1, loops_blocked=0,
        boundary_edges_in=12, boundary_edges_out=7, boundary_groups_out=1, longest_filled=5, nonmanifold_edges=0)
