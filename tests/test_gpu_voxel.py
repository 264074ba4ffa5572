"""p2s_mesh_voxelize on the device (TriMesh.voxelize) against the two CPU models (tests/voxel_model.py): the walk of the
octree against the exhaustive kernel, the occupancy against exact rationals, flags and report against the float64
restatement of the rules, the capacity and the closedness rule with sentinel buffers, and the three fixture meshes against
the signed distance (another kernel path)."""
import ctypes

import numpy as np
import pytest
import torch

import voxel_model as M
from test_mesh_sdf_model import MESHES, load
from test_voxel_model import CASES, exact_of

pytestmark = pytest.mark.gpu

P2S_EINVAL, P2S_ECAPACITY = -1, -4
SENTINEL = 0xA5


def _trimesh(v, f):
    from points2surf_amd import gt_sdf
    return gt_sdf.TriMesh(np.asarray(v, np.float32), np.asarray(f, np.int32))


def _voxelize(mesh, res, method, **kw):
    occ, flags, rep = mesh.voxelize(res, method=method, want_flags=True, want_report=True, **kw)
    return occ.cpu().numpy(), flags.cpu().numpy(), rep


def _both(mesh, res, **kw):
    """index == exhaustive in occ, flags and report except the tests; returns the index's result"""
    a, b = _voxelize(mesh, res, 'index', **kw), _voxelize(mesh, res, 'exhaustive', **kw)
    assert a[0].dtype == np.uint8 and a[0].shape == (res, res, res) and a[1].shape == (res, res, res)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in M.REPORT_KEYS:
        assert k == 'tests' or a[2][k] == b[2][k], (k, a[2], b[2])
    assert a[2]['tests'] <= b[2]['tests'] == res * res * mesh.info()['n_faces']
    return a


def _raw(mesh, res, method, max_fallback, occ, flags):
    """the C call on buffers of the caller: (return code, report)"""
    from points2surf_amd import engine
    rep = (ctypes.c_int64 * 8)()
    rc = mesh.lib.p2s_mesh_voxelize(mesh.handle, res, method, max_fallback, engine._ptr(occ), engine._ptr(flags), rep,
                                    engine._stream_ptr(mesh.device))
    torch.cuda.synchronize()
    return rc, [int(x) for x in rep]


@pytest.mark.parametrize('name', sorted(CASES))
def test_constructions_match_both_models(name):
    build, res, inside, on_surface = CASES[name]
    v, f = build()
    mesh = _trimesh(v, f)
    try:
        occ, flags, rep = _both(mesh, res)
    finally:
        mesh.close()
    print(name, rep)
    w, on = exact_of(name)
    assert int(on.sum()) == on_surface                       # the voxels left out of the comparison: 0, or the 8 corners
    assert np.array_equal(occ[~on], (w != 0)[~on].astype(np.uint8))
    want = M.kernel(v, f, res)
    assert np.array_equal(flags, want['flags'])
    assert rep == dict(want['report'], tests=rep['tests'])
    assert np.array_equal(occ, want['occ'])
    if on_surface == 0:
        assert rep['inside'] == inside == int(occ.sum())


def test_inward_mesh_is_voxelised_as_stored():
    v, f = M.cube(0.3, inward=True)
    mesh = _trimesh(v, f)
    try:
        assert mesh.info()['inverted']
        occ, flags, rep = _both(mesh, 8)
    finally:
        mesh.close()
    want = M.kernel(*M.cube(0.3), 8)
    assert np.array_equal(occ, want['occ']) and rep['inside'] == 8


def test_smallest_grid():
    v, f = M.cube(0.3)
    mesh = _trimesh(v, f)
    try:
        occ, flags, rep = _both(mesh, 2)                     # centres +-0.5: all outside
    finally:
        mesh.close()
    want = M.kernel(v, f, 2)
    assert not occ.any() and np.array_equal(flags, want['flags']) and rep == dict(want['report'], tests=rep['tests'])


def test_largest_grid_by_the_walk():
    """R = 1024, 2^30 voxels, the walk only: the cube is the product of its three 1-D intervals.  The columns on the faces'
    diagonal x = y inside the cube go to the exact sum: max_fallback is set to exactly what they need."""
    v, f = M.cube(0.3)
    c = torch.from_numpy(M.centres(1024)).cuda()
    m = (c.abs() < float(np.float32(0.3)))
    n_in = int(m.sum())
    mesh = _trimesh(v, f)
    try:
        occ, rep = mesh.voxelize(1024, max_fallback=n_in * 1024, want_report=True)
    finally:
        mesh.close()
    print('R = 1024', rep)
    assert rep['undecided_columns'] == n_in and rep['undecided_voxels'] == 0 and rep['fallback'] == n_in * 1024
    assert rep['inside'] == n_in ** 3 and rep['crossings'] == 2 * (n_in * n_in - n_in)
    want = (m[:, None, None] & m[None, :, None] & m[None, None, :]).to(torch.uint8)
    assert torch.equal(occ, want)


def test_capacity_rule_leaves_the_outputs_untouched():
    """octahedron at R = 5: 9 undecided columns, U = 45; max_fallback 45 is enough, 44 is P2S_ECAPACITY with the report
    filled and nothing written"""
    v, f = M.octahedron(0.9)
    mesh = _trimesh(v, f)
    try:
        for method in (0, 1):
            occ = torch.full((5, 5, 5), SENTINEL, dtype=torch.uint8, device='cuda')
            flags = torch.full((5, 5, 5), SENTINEL, dtype=torch.uint8, device='cuda')
            rc, rep = _raw(mesh, 5, method, 44, occ, flags)
            assert rc == P2S_ECAPACITY and rep[1] == 9 and rep[2] == 0 and rep[3] == 45
            assert bool((occ == SENTINEL).all()) and bool((flags == SENTINEL).all())
            rc, rep = _raw(mesh, 5, method, 45, occ, flags)
            assert rc == 0 and rep[0] == 25 and rep[1] == 9 and rep[3] == 45
            assert int(occ.sum()) == 25 and int(flags.sum()) == 45
        from points2surf_amd import _lib
        with pytest.raises(_lib.P2SError) as e:
            mesh.voxelize(5, max_fallback=44)
        assert e.value.code == P2S_ECAPACITY and mesh.voxel_report['fallback'] == 45
    finally:
        mesh.close()


def test_open_mesh_and_bad_arguments_are_refused_untouched():
    mesh = _trimesh(*M.open_cube(0.3))
    closed = _trimesh(*M.cube(0.3))
    try:
        assert not mesh.closed
        occ = torch.full((8, 8, 8), SENTINEL, dtype=torch.uint8, device='cuda')
        for method in (0, 1):
            rc, rep = _raw(mesh, 8, method, 1 << 20, occ, None)
            assert rc == P2S_EINVAL and rep == [0] * 8 and bool((occ == SENTINEL).all())
        for res, method, cap in ((1, 0, 10), (1025, 0, 10), (8, 2, 10), (8, 0, -1)):
            rc, rep = _raw(closed, res, method, cap, occ, None)
            assert rc == P2S_EINVAL and bool((occ == SENTINEL).all())
    finally:
        mesh.close()
        closed.close()


@pytest.mark.parametrize('name', MESHES)
def test_fixture_meshes_against_the_signed_distance(name):
    """R = 32: the walk == the exhaustive kernel, and occ == (signed distance > 0) wherever |d| > 1e-6: the pseudonormal /
    per-component sign is another kernel path.  Fewer than 1 % of the centres may lie that close to the surface."""
    v, f = load(name)[:2]
    res = 32
    mesh = _trimesh(v, f)
    try:
        occ, flags, rep = _both(mesh, res)
        c = torch.from_numpy(M.centres(res)).cuda()
        q = torch.stack(torch.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3)
        d = mesh.distance(q, signed=True).cpu().numpy().reshape(res, res, res)
    finally:
        mesh.close()
    print(name, rep)
    far = np.abs(d) > 1e-6
    assert (~far).sum() < 0.01 * res ** 3
    assert np.array_equal(occ[far], (d > 0)[far].astype(np.uint8))
    assert rep['inside'] == int(occ.sum()) and rep['fallback'] == int(flags.sum())
    assert rep['tests'] < res * res * len(f)
