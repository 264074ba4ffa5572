"""CPU model of the reductions and the formulas of metrics.mesh_quality (p2s_surface_stats, p2s_occupancy_counts): numpy
float64 on the same per-sample arrays, and what two concentric axis cubes must give."""
import numpy as np

DEGENERATE_REL = 2.0 ** -90


def unit_normals(verts, faces):
    """[F, 3] float64 unit normals of the float32 mesh; 0 for a face under the degenerate rule.  (The handle computes them in
    another operation order: a component may differ by a few units of 2^-53.)"""
    T = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces)]
    ab, ac = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    n = np.cross(ab, ac)
    nn = (n * n).sum(1)
    ok = nn > DEGENERATE_REL * ((ab * ab).sum(1) * (ac * ac).sum(1))
    out = np.zeros_like(n)
    out[ok] = n[ok] / np.sqrt(nn[ok])[:, None]
    return out


def surface_stats(dist, face_from, face_to, normals_from, normals_to, taus):
    """dict as metrics.surface_stats returns it"""
    d = np.asarray(dist, np.float64)
    a, b = normals_from[np.asarray(face_from)], normals_to[np.asarray(face_to)]
    keep = (a != 0).any(1) & (b != 0).any(1)
    return dict(sum=float(d.sum()), sum_sq=float((d * d).sum()), max=float(d.max()) if len(d) else 0.0,
                sum_nc=float(np.abs((a[keep] * b[keep]).sum(1)).sum()), nc_pairs=int(keep.sum()),
                counts=[int((d <= t).sum()) for t in taus])


def summary(new_to_ref, ref_to_new, n, taus):
    """the distance, F-score and normal entries of mesh_quality from the two directed stats"""
    out = {}
    for name, st in (('accuracy', new_to_ref), ('completeness', ref_to_new)):
        out[name + '_mean'], out[name + '_rms'], out[name + '_max'] = st['sum'] / n, float(np.sqrt(st['sum_sq'] / n)), st['max']
    out['chamfer_l1'] = (out['accuracy_mean'] + out['completeness_mean']) / 2.0
    out['hausdorff'] = max(out['accuracy_max'], out['completeness_max'])
    for k, t in enumerate(taus):
        p, r = new_to_ref['counts'][k] / n, ref_to_new['counts'][k] / n
        out['precision@%g' % t], out['recall@%g' % t] = p, r
        out['fscore@%g' % t] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    out['normal_consistency'] = (new_to_ref['sum_nc'] / new_to_ref['nc_pairs'] + ref_to_new['sum_nc'] / ref_to_new['nc_pairs']) / 2.0
    return out


def occupancy_counts(occ_a, occ_b):
    a, b = np.asarray(occ_a) != 0, np.asarray(occ_b) != 0
    return int(a.sum()), int(b.sum()), int((a & b).sum())


def iou(occ_a, occ_b):
    na, nb, nab = occupancy_counts(occ_a, occ_b)
    return nab / float(na + nb - nab) if na + nb - nab else -1.0


def box_distance(points, half):
    """the exact distance of points ON OR OUTSIDE the axis cube |x|, |y|, |z| <= half to it (float64)"""
    e = np.maximum(np.abs(np.asarray(points, np.float64)) - np.float64(half), 0.0)
    return np.sqrt((e * e).sum(1))
