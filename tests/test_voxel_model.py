"""CPU: the two models of p2s_mesh_voxelize (tests/voxel_model.py) against counts derived by hand, and against each other.

The hand counts.  The centres of R voxels per axis are (2 i + 1) / R - 1.
 * axis cube, half-side float32(0.3) (just above 0.3): R = 8 has the centres +-0.125 inside per axis, 2^3 = 8; R = 6 has
   +-1/6, again 8; nothing on the surface.
 * half-side 0.25 at R = 4: the centres are +-0.25, +-0.75, so the 8 voxels (+-0.25)^3 ARE the corners: on the surface;
   no centre lies strictly inside.
 * octahedron |x| + |y| + |z| < float32(0.9) (just below 0.9): R = 4, centres +-0.25, +-0.75: only (+-0.25)^3 (sum 0.75): 8.
   R = 5, centres 0, +-0.4, +-0.8: all three 0 (1); two 0 and one +-0.4 or +-0.8 (3 * 4 = 12); one 0 and two +-0.4
   (3 * 4 = 12); 0.4 + 0.4 + 0.4 = 1.2 and 0.8 + 0.4 are outside: 25.  Its edges project onto the lines x = 0, y = 0 and
   |x| + |y| = 0.9; the columns with x = 0 or y = 0 are 5 + 5 - 1 = 9.
 * cube 0.4 with an inward cube 0.2 inside, R = 8: +-0.125, +-0.375 per axis inside the outer (64), +-0.125 inside the
   cavity (8): 56.
 * two outward cubes of half-side 0.3 at x = -+0.15, R = 8: x in (-0.45, 0.45): 4 centres, y and z 2 each: 16 inside; the
   overlap |x| < 0.15: 2 * 2 * 2 = 8 voxels with w = 2."""
import numpy as np
import pytest

import voxel_model as M

# name -> (mesh, R, voxels inside, voxels on the surface)
CASES = {
    'cube_r8': (lambda: M.cube(0.3), 8, 8, 0),
    'cube_r6': (lambda: M.cube(0.3), 6, 8, 0),
    'cube_corners_r4': (lambda: M.cube(0.25), 4, 0, 8),
    'octahedron_r4': (lambda: M.octahedron(0.9), 4, 8, 0),
    'octahedron_r5': (lambda: M.octahedron(0.9), 5, 25, 0),
    'cavity_r8': (M.cube_with_cavity, 8, 56, 0),
    'two_cubes_r8': (M.two_cubes, 8, 16, 0),
}
_EXACT = {}


def exact_of(name):
    """the exact model of a case, computed once and shared (read only)"""
    if name not in _EXACT:
        mesh, res = CASES[name][0](), CASES[name][1]
        w, on = M.exact(mesh[0], mesh[1], res)
        w.setflags(write=False)
        on.setflags(write=False)
        _EXACT[name] = (w, on)
    return _EXACT[name]


def test_centres_are_the_float32_of_the_float64_expression():
    c = M.centres(5)
    assert c.dtype == np.float32 and c[2] == 0.0
    assert [float(x) for x in c] == [float(np.float32(v)) for v in (-0.8, -0.4, 0.0, 0.4, 0.8)]
    assert np.array_equal(M.centres(4), np.array([-0.75, -0.25, 0.25, 0.75], np.float32))
    assert abs(float(M.centres(1024)[-1])) < 1.0


@pytest.mark.parametrize('name', sorted(CASES))
def test_exact_model_gives_the_hand_counts(name):
    _, res, inside, on_surface = CASES[name]
    w, on = exact_of(name)
    assert int(on.sum()) == on_surface
    assert int(((w != 0) & ~on).sum()) == inside
    assert w.min() >= 0                                      # outward shells, and a cavity inside one


def test_the_corners_of_the_r4_cube_are_the_surface_voxels():
    _, on = exact_of('cube_corners_r4')
    want = np.zeros((4, 4, 4), bool)
    want[1:3, 1:3, 1:3] = True
    assert np.array_equal(on, want)


def test_overlap_has_winding_two_and_cavity_zero():
    w, _ = exact_of('two_cubes_r8')
    assert int((w == 2).sum()) == 8 and int((w == 1).sum()) == 8 and (w[3:5, 3:5, 3:5] == 2).all()
    w, _ = exact_of('cavity_r8')
    assert (w[3:5, 3:5, 3:5] == 0).all() and int((w == 1).sum()) == 56


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_model_agrees_with_the_exact_model(name):
    mesh, res, inside, on_surface = CASES[name][0](), *CASES[name][1:]
    k = M.kernel(mesh[0], mesh[1], res)
    w, on = exact_of(name)
    assert np.array_equal(k['occ'][~on], (w != 0)[~on].astype(np.uint8))
    r = k['report']
    assert r['fallback'] == r['undecided_columns'] * res + r['undecided_voxels'] == int(k['flags'].sum())
    assert k['flags'][on].all()                              # a voxel on the surface is never decided by the columns
    if on_surface == 0:
        assert r['inside'] == inside
    assert r['tests'] == res * res * len(mesh[1])


def test_octahedron_r5_columns():
    """9 columns run through a vertex or along a projected edge (x = 0 or y = 0); no other voxel is undecided: U = 45"""
    v, f = M.octahedron(0.9)
    k = M.kernel(v, f, 5)
    assert k['report']['undecided_columns'] == 9 and k['report']['undecided_voxels'] == 0 and k['report']['fallback'] == 45
    col = k['flags'].all(2)
    want = np.zeros((5, 5), bool)
    want[2, :] = want[:, 2] = True
    assert np.array_equal(col, want) and np.array_equal(k['flags'].any(2), want)


def test_cube_columns_on_the_face_diagonals_are_undecided():
    """the top and the bottom face are split along x = y: the two columns (+-0.125, +-0.125) on it go to the exact sum; the
    side faces are seen edge-on, and every column is strictly clear of them (outside their boxes)"""
    v, f = M.cube(0.3)
    k = M.kernel(v, f, 8)
    assert k['report']['undecided_columns'] == 2 and k['flags'][3, 3].all() and k['flags'][4, 4].all()
    assert k['report']['crossings'] == 2 * 2 + 2 * 0           # the two decided columns inside cross top and bottom
    assert k['report']['inside'] == 8


def test_stored_flips_an_inward_mesh():
    v, f = M.cube(0.3, inward=True)
    T = M.stored(v, f)
    assert np.einsum('ij,ij->i', T[:, 0], np.cross(T[:, 1], T[:, 2])).sum() > 0
    assert np.array_equal(T, M.stored(*M.cube(0.3))[:, [2, 1, 0]][:, [0, 2, 1]])
