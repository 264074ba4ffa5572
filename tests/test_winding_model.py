"""The float64 CPU model of the winding-number kernels (tests/winding_model.py): the bound of a node taken as a dipole, the
exact sum on the closed fixture meshes, and the ctypes prototype of p2s_mesh_winding against the header.  No device."""
import ctypes
import os
import re

import numpy as np

import winding_model as wm
from test_mesh_sdf_model import MESHES, load

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bound_lemma_on_random_clusters():
    """|exact - dipole| <= A r / (2 pi (d - r)^3): 2,000 clusters of 1..64 triangles, d / r log-uniform in [1.01, 100]"""
    rng = np.random.RandomState(20130721)
    worst = 0.0
    for k in range(2000):
        t = rng.randint(1, 65)
        size = 10.0 ** rng.uniform(-2, 0)
        tris = rng.uniform(-1, 1, 3) + rng.uniform(-size, size, (t, 1, 3)) + rng.uniform(-size, size, (t, 3, 3)) * rng.uniform(0.05, 1)
        c, r = wm.box_of(tris)
        ratio = 1.01 * (100.0 / 1.01) ** rng.uniform(0, 1)
        u = rng.normal(size=3)
        p = c + (ratio * r) * u / np.sqrt((u * u).sum())
        exact, dipole, bound = wm.cluster(tris, c, r, p)
        assert np.isfinite([exact, dipole, bound]).all()
        assert abs(exact - dipole) <= bound, (k, t, ratio, exact, dipole, bound)
        worst = max(worst, abs(exact - dipole) / bound)
    print('largest |exact - dipole| / bound', worst)
    assert worst > 1e-3                                   # the bound is not vacuous


def test_moments_skip_degenerate_faces():
    tris = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [1, 0, 0], [2, 0, 0]], [[3, 3, 3]] * 3], np.float64)
    N, A, deg = wm.moments(tris)
    assert np.array_equal(N, [0, 0, 0.5]) and A == 0.5 and deg == 2


def test_exact_sum_is_an_integer_on_the_closed_fixtures():
    for name in MESHES:
        v, f, q, _ = load(name)
        w = wm.winding_exact(v, f, q)
        dev = np.abs(w - np.round(w)).max()
        print(name[:8], 'max |w - round(w)|', dev, 'values', np.unique(np.round(w)))
        assert len(q) == 2000 and dev <= 1e-12


C_TYPES = {'p2s_trimesh_t': ctypes.c_void_p, 'const float *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int,
           'double': ctypes.c_double, 'double *': ctypes.c_void_p, 'int64_t *': ctypes.POINTER(ctypes.c_int64),
           'void *': ctypes.c_void_p}


def test_ctypes_prototype_matches_the_header():
    from points2surf_amd import _lib
    src = open(os.path.join(REPO, 'include', 'p2s_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+p2s_mesh_winding\s*\(([^)]*)\)\s*;', src)
    assert m, 'p2s_mesh_winding is not declared in include/p2s_hip.h'
    args = []
    for a in m.group(1).split(','):
        a = ' '.join(a.split())
        name = re.search(r'([A-Za-z_][A-Za-z0-9_]*)$', a).group(1)
        args.append(a[:-len(name)].strip())
    assert args == ['p2s_trimesh_t', 'const float *', 'int64_t', 'int', 'double', 'double *', 'double *', 'int64_t *', 'void *']
    res, argtypes = _lib.PROTOTYPES['p2s_mesh_winding']
    assert res is ctypes.c_int and argtypes == [C_TYPES[a] for a in args]
    assert re.search(r'#define\s+P2S_ABI_VERSION\s+5\b', open(os.path.join(REPO, 'include', 'p2s_hip.h')).read())
