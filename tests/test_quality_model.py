"""CPU: the model of the quality report's reductions and formulas (tests/quality_model.py) against values derived by hand."""
import numpy as np

import quality_model as Q
import voxel_model as V

DELTA = 1.0 / 64.0


def test_unit_normals_and_the_degenerate_rule():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0], [4, 0, 0]], np.float32)
    n = Q.unit_normals(v, np.array([[0, 1, 2], [0, 2, 1], [0, 1, 3]]))
    assert np.array_equal(n, np.array([[0, 0, 1.0], [0, 0, -1.0], [0, 0, 0]]))


def test_surface_stats_by_hand():
    n_from = np.array([[0, 0, 1.0], [0, 0, 0]])
    n_to = np.array([[0, 0.6, -0.8], [1.0, 0, 0]])
    st = Q.surface_stats([0.0, 0.25, 0.5, 1.0], [0, 0, 1, 0], [0, 1, 0, 0], n_from, n_to, (0.25, 0.75, 2.0))
    assert st == dict(sum=1.75, sum_sq=0.0625 + 0.25 + 1.0, max=1.0, sum_nc=0.8 + 0.0 + 0.8, nc_pairs=3, counts=[2, 3, 4])


def test_summary_formulas():
    a = dict(sum=2.0, sum_sq=2.0, max=1.5, sum_nc=3.0, nc_pairs=4, counts=[4, 0])
    b = dict(sum=4.0, sum_sq=8.0, max=0.5, sum_nc=2.0, nc_pairs=2, counts=[2, 0])
    s = Q.summary(a, b, 4.0, (0.5, 0.125))
    assert (s['accuracy_mean'], s['completeness_mean'], s['chamfer_l1'], s['hausdorff']) == (0.5, 1.0, 0.75, 1.5)
    assert s['accuracy_rms'] == np.sqrt(0.5) and s['completeness_rms'] == np.sqrt(2.0)
    assert (s['precision@0.5'], s['recall@0.5']) == (1.0, 0.5) and abs(s['fscore@0.5'] - 2.0 / 3.0) < 1e-15
    assert s['fscore@0.125'] == 0.0                           # P + R = 0
    assert s['normal_consistency'] == (0.75 + 1.0) / 2.0


def test_concentric_cubes_by_hand():
    """every point of the inner cube's surface lies delta from the outer one's; an outer corner lies delta sqrt(3) from the
    inner cube; at R = 16 the centres +-0.0625, +-0.1875 lie inside both (0.3 and 0.3 - 1/64), +-0.3125 inside neither"""
    outer = np.float32(0.3)
    inner = np.float32(outer - np.float32(DELTA))
    assert float(outer) - float(inner) == DELTA                # the subtraction is exact in float32
    corners = V.cube(outer)[0]
    assert np.abs(Q.box_distance(corners, inner) - DELTA * np.sqrt(3.0)).max() < 1e-15
    occ = [(V.exact(*V.cube(h), 16)[0] != 0) for h in (outer, inner)]
    assert Q.occupancy_counts(*occ) == (64, 64, 64) and Q.iou(*occ) == 1.0
    assert Q.iou(np.zeros(8), np.zeros(8)) == -1.0
    assert Q.iou([1, 1, 0, 0], [0, 1, 1, 1]) == 0.25
