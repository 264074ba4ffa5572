"""CPU: the numpy model of the quadric vertex clustering (tests/simplify_model.py; include/p2s_hip.h: p2s_mesh_simplify)
pinned on cases whose answer is known without it."""
import time

import numpy as np
import pytest

import simplify_model as SM


@pytest.fixture(scope='module')
def cube():
    return SM.cube(24)


def test_a_grid_finer_than_the_mesh_changes_nothing():
    """R so large that no two vertices share a cell: the faces and the referenced vertices come back as they went in"""
    v, f = SM.torus(12, 6)
    v = np.concatenate([v, [[0.0, 0.0, 0.4]]]).astype(np.float32)          # a vertex no face uses
    lin = SM.cells(v, 1024)[1]
    assert np.unique(lin).size == v.shape[0]
    for placement in ('mean', 'quadric'):
        out = SM.simplify(v, f, resolution=1024, placement=placement)
        assert np.array_equal(out['faces'], f) and np.array_equal(out['face_src'], np.arange(len(f)))
        assert np.array_equal(out['vert_map'], np.r_[np.arange(len(v) - 1), -1])
        r = out['report']
        assert (r[1], r[2], r[3], r[4], r[5], r[6]) == (len(v) - 1, len(f), 1024, len(v), 0, 0)
        if placement == 'mean':
            assert out['verts'].tobytes() == v[:-1].tobytes()               # one vertex per cell: g + (p - g), Sterbenz-exact
        else:                                                               # the vertex lies on all its planes: A m + r ~ 0
            assert np.abs(out['verts'].astype(np.float64) - v[:-1]).max() <= 1e-3 * out['h']
        assert r[12] == r[13] == 0


@pytest.mark.parametrize('R', [6, 8])
def test_quadric_placement_finds_the_cube_corners(cube, R):
    v, f = cube
    assert f.shape[0] == 12 * 24 * 24 and v.shape[0] == 6 * 24 * 24 + 2
    assert SM.edge_word(f) == 0
    q = SM.simplify(v, f, resolution=R, placement='quadric')
    m = SM.simplify(v, f, resolution=R, placement='mean')
    h = q['h']
    assert h == 1.0 / R
    dq, dm = SM.corner_distances(q['verts'], h), SM.corner_distances(m['verts'], h)
    print('R = %d: corners at %.4f .. %.4f h (quadric), %.3f .. %.3f h (mean); largest max|x|/h %.3f'
          % (R, dq.min(), dq.max(), dm.min(), dm.max(), np.nanmax(q['ratio'])))
    assert (dq < 0.01).all(), dq
    assert (dm > 0.1).all(), dm
    assert np.array_equal(q['faces'], m['faces']) and q['report'][10] == 0 and q['report'][9] == 0
    assert q['report'][8] == q['report'][1]


def test_the_search_is_its_loop():
    v, f = SM.torus(48, 20)
    for max_faces in (0, 7, 300, 1000, len(f) - 1):
        counted = {}

        def count(R):
            counted[R] = SM.surviving(v, f, R)
            return counted[R]
        R, probes = SM.search_resolution(v, f, max_faces, count)
        assert probes == len(counted) == 10                        # 1024 = 2^10 candidates
        assert counted.get(R, 0 if R == 1 else None) <= max_faces
        # replay: every probe moved the bracket as the loop says
        lo, hi = 1, 1024
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if counted[mid] <= max_faces else (lo, mid - 1)
        assert lo == R
        out = SM.simplify(v, f, max_faces=max_faces)
        assert out['report'][3] == R and out['report'][11] == 10 and out['report'][2] <= max_faces
        assert out['report'][2] + out['report'][6] == SM.surviving(v, f, R)
    assert SM.surviving(v, f, 1) == 0                              # R = 1 always qualifies
    out = SM.simplify(v, f, max_faces=len(f))                      # nothing to do: the input, bit for bit
    assert out['verts'].tobytes() == v.tobytes() and out['faces'].tobytes() == f.tobytes() and out['report'][3] == 0
    assert out['report'][11] == 0 and np.array_equal(out['vert_map'], np.arange(len(v)))


def test_points_on_cell_boundaries_and_on_the_upper_bound():
    """min(R - 1, floor((p - lo) * (R / ext))): a point on a boundary belongs to the upper cell, the box's upper bound to
    the last cell"""
    v = np.array([[0, 0, 0], [4, 4, 4], [1, 2, 3], [0.999999, 2.0, 3.999], [4, 0, 2], [2, 2, 2]], np.float32)
    idx, lin = SM.cells(v, 4)
    assert idx.tolist() == [[0, 0, 0], [3, 3, 3], [1, 2, 3], [0, 2, 3], [3, 0, 2], [2, 2, 2]]
    assert lin.tolist() == [0, 63, 27, 11, 50, 42]
    idx, _ = SM.cells(v - np.float32(2.0), 4)                       # lo = -2: the same cells
    assert idx.tolist() == [[0, 0, 0], [3, 3, 3], [1, 2, 3], [0, 2, 3], [3, 0, 2], [2, 2, 2]]
    flat = np.zeros((3, 3), np.float32) + np.float32(0.25)          # ext = 0: every vertex in cell 0
    assert SM.cells(flat, 7)[1].tolist() == [0, 0, 0]
    out = SM.simplify(flat, [[0, 1, 2]], resolution=7)
    assert out['report'][1] == 0 and out['report'][2] == 0 and out['report'][5] == 1 and out['vert_map'].tolist() == [-1, -1, -1]


def test_the_grid_is_that_of_the_voxel_thinning():
    import prepare_model as PM
    p = PM.seeded_cloud(4099)                                       # both signs, exact +-0, repeated values
    for R in (1, 7, 64, 1024):
        assert np.array_equal(SM.cells(p, R)[1], PM.voxel_cells(p, R)[0])


def test_faces_of_one_vertex_set_keep_the_smallest_id():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1], [0.01, 0.01, 0.0], [0.98, 0.0, 0.02]], np.float32)
    f = np.array([[3, 1, 2], [0, 1, 2], [2, 4, 5], [1, 0, 2], [0, 4, 1], [5, 2, 0]], np.int32)
    # R = 2: vertices 0 and 4 share a cell, 1 and 5 too; faces 1, 2, 3, 5 become the set {0, 1, 2}; face 4 collapses
    out = SM.simplify(v, f, resolution=2, placement='mean')
    assert out['vert_map'].tolist() == [0, 1, 2, 3, 0, 1]
    assert out['face_src'].tolist() == [0, 1] and out['faces'].tolist() == [[3, 1, 2], [0, 1, 2]]
    r = out['report']
    assert (r[1], r[2], r[5], r[6]) == (4, 2, 1, 3)
    assert np.allclose(out['verts'][0], [0.005, 0.005, 0.0], atol=1e-7) and np.allclose(out['verts'][1], [0.99, 0.0, 0.01], atol=1e-7)


def test_degenerate_faces_contribute_no_quadric():
    v = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1], [0.02, 0.02, 0.02]], np.float32)
    f = np.array([[0, 1, 2], [3, 1, 2]], np.int32)
    out = SM.simplify(v, f, resolution=4, placement='quadric')
    r = out['report']
    assert (r[2], r[7], r[8], r[9], r[10]) == (1, 2, 0, 3, 0)       # the second face is a duplicate set; tr(A) = 0: the mean
    assert out['verts'].tobytes() == SM.simplify(v, f, resolution=4, placement='mean')['verts'].tobytes()


def test_model_time_on_a_20k_face_mesh_is_context_only():
    v, f = SM.torus()
    t0 = time.perf_counter()
    out = SM.simplify(v, f, resolution=64)
    print('numpy model, torus of %d faces at R = 64: %.0f ms (context only), %d occupied cells, largest max|x|/h %.3f'
          % (len(f), (time.perf_counter() - t0) * 1e3, out['report'][4], np.nanmax(out['ratio'])))
    assert len(f) == 20480 and out['report'][2] <= SM.surviving(v, f, 64)
