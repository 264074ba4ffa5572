"""Mesh metrics on the device: what reference source/base/evaluation.py:222-392 computes with trimesh +
scipy on the host -- even surface samples of the reconstructed and the reference mesh, Hausdorff and Chamfer distances
between the sample sets -- through libp2s_hip.so (p2s_mesh_sample_surface, p2s_points_remove_close,
p2s_nn_distance_stats).  Torch tensors are containers only; no CPU fallback.

The reference samples with numpy's unseeded global generator (trimesh.sample.sample_surface -> np.random.random), so
its numbers change from run to run; here the deviates come from a seeded device twin of ``np.random.RandomState``
(``seed`` argument), in the order trimesh draws them.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import ply as _ply


def _dev(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError('points2surf_amd needs a ROCm GPU (gfx950); no CPU fallback exists')
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def sample_surface(verts, faces, count, rng, want_faces=False):
    """trimesh.sample.sample_surface(mesh, count): (points [count,3] float32 device tensor, area)"""
    lib = _lib.load()
    dev = verts.device
    v = verts.to(dev, torch.float32).contiguous()
    f = faces.to(dev, torch.int32).contiguous()
    u = torch.empty((3 * count,), dtype=torch.float64, device=dev)
    pts = torch.empty((count, 3), dtype=torch.float32, device=dev)
    fid = torch.empty((count,), dtype=torch.int32, device=dev) if want_faces else None
    area = ctypes.c_double(0.0)
    with torch.cuda.device(dev):
        s = _engine._stream_ptr(dev)
        _lib.check(lib.p2s_rng_random_sample(rng.handle, 3 * count, _engine._ptr(u), s))
        _lib.check(lib.p2s_mesh_sample_surface(_engine._ptr(v), _engine._ptr(f), int(f.shape[0]), _engine._ptr(u), int(count),
                                               _engine._ptr(pts), _engine._ptr(fid), ctypes.byref(area), dev.index, s))
    return (pts, float(area.value), fid) if want_faces else (pts, float(area.value))


def sample_surface_even(verts, faces, count, rng):
    """trimesh.sample.sample_surface_even(mesh, count) (reference source/base/evaluation.py:235): 3 * count area-weighted
    samples, minus the points with a neighbour within sqrt(area / (3 count)), cut to count.  Returns [<= count, 3]."""
    lib = _lib.load()
    dev = verts.device
    cand, area = sample_surface(verts, faces, 3 * count, rng)
    radius = float(np.sqrt(area / (3 * count)))
    out = torch.empty((count, 3), dtype=torch.float32, device=dev)
    n = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        _lib.check(lib.p2s_points_remove_close(_engine._ptr(cand), int(cand.shape[0]), ctypes.c_double(radius), int(count),
                                               _engine._ptr(out), ctypes.byref(n), dev.index, _engine._stream_ptr(dev)))
    return out[:n.value]


def directed_stats(samples_from, samples_to):
    """(max, sum) of the nearest-neighbour distances from every point of ``samples_from`` to the set ``samples_to``:
    scipy.spatial.distance.directed_hausdorff(from, to)[0] and the Chamfer term np.sum(kdtree_to.query(from)[0])"""
    lib = _lib.load()
    target = _engine.Cloud(samples_to)
    q = samples_from.to(target.device, torch.float32).contiguous()
    mx, sm = ctypes.c_double(0.0), ctypes.c_double(0.0)
    with torch.cuda.device(target.device):
        _lib.check(lib.p2s_nn_distance_stats(target.handle, _engine._ptr(q), int(q.shape[0]), None, ctypes.byref(mx),
                                             ctypes.byref(sm), _engine._stream_ptr(target.device)))
    target.close()
    return float(mx.value), float(sm.value)


def mesh_distances(file_in, file_ref, samples_per_model=10000, seed=0, device=None):
    """(hausdorff new->ref, hausdorff ref->new, hausdorff, chamfer) of two mesh files; (-1, -1, -1, -1) if a mesh is
    missing or empty (reference :244-245, :278-279, :298-299)"""
    dev = _dev(device)
    sets = []
    rng = _engine.Rng(seed, device=dev)
    for path in (file_in, file_ref):
        try:
            v, f = _ply.read_ply(path)
        except Exception:
            v, f = np.zeros((0, 3)), np.zeros((0, 3), np.int64)
        if v.shape[0] == 0 or f.shape[0] == 0:
            return -1.0, -1.0, -1.0, -1.0
        f = np.asarray(f)
        if f.ndim != 2 or f.shape[1] != 3 or f.min() < 0 or f.max() >= v.shape[0] or not np.isfinite(v).all():
            # malformed / truncated mesh: the reference's try/except around trimesh ends in (-1, -1, -1, -1)
            # (source/base/evaluation.py:244-245); never hand out-of-range indices to the device kernels
            return -1.0, -1.0, -1.0, -1.0
        vt = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
        ft = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).to(dev)
        s = sample_surface_even(vt, ft, samples_per_model, rng)
        if s.shape[0] == 0:
            return -1.0, -1.0, -1.0, -1.0
        sets.append(s)
    new, ref = sets
    h_nr, s_nr = directed_stats(new, ref)
    h_rn, s_rn = directed_stats(ref, new)
    return h_nr, h_rn, max(h_nr, h_rn), s_nr + s_rn


def _pairing(new_meshes_dir_abs, ref_meshes_dir_abs, dataset_file_abs):
    """the pairing rules of reference source/base/evaluation.py:307-392, shared by mesh_comparison and quality_comparison:
    rows (new file, ref file, code) in the order the reference appends them -- code 0: compare the two; -2: a
    reconstruction outside the set to compare that has a reference (no data set file only); -1: in the set to compare,
    never reconstructed.  No row of code 0: ValueError('Results are empty!')."""
    new_mesh_files = sorted(f for f in os.listdir(new_meshes_dir_abs) if os.path.isfile(os.path.join(new_meshes_dir_abs, f)))
    ref_mesh_files = sorted(f for f in os.listdir(ref_meshes_dir_abs) if os.path.isfile(os.path.join(ref_meshes_dir_abs, f)))
    if dataset_file_abs is None:
        to_compare = set(ref_mesh_files)
    else:
        if not os.path.isfile(dataset_file_abs):
            raise ValueError('File does not exist: {}'.format(dataset_file_abs))
        with open(dataset_file_abs) as f:
            to_compare = set((line.replace('\n', '') + '.ply').split('.')[0] for line in f.readlines())

    def ref_for(new_mesh_file):
        stem = new_mesh_file.split('.')[0]
        return sorted(set(f for f in ref_mesh_files if f.split('.')[0] == stem))

    rows = []
    for new_mesh_file in new_mesh_files:
        if new_mesh_file.split('.')[0] in to_compare:
            match = ref_for(new_mesh_file)
            if match:
                rows.append((os.path.join(new_meshes_dir_abs, new_mesh_file), os.path.join(ref_meshes_dir_abs, match[0]), 0))
    if len(rows) == 0:
        raise ValueError('Results are empty!')
    for new_mesh_file in new_mesh_files:          # no reference but reconstruction
        stem = new_mesh_file.split('.')[0]
        if stem not in to_compare:
            if dataset_file_abs is None:
                match = ref_for(new_mesh_file)
                if match:
                    rows.append((os.path.join(new_meshes_dir_abs, new_mesh_file),
                                 os.path.join(ref_meshes_dir_abs, match[0]), -2))
        else:
            to_compare.remove(stem)
    for missing in sorted(to_compare):            # no reconstruction but reference
        rows.append((os.path.join(new_meshes_dir_abs, missing), os.path.join(ref_meshes_dir_abs, missing), -1))
    return rows


def _write_csv(report_name, header, results):
    if os.path.dirname(report_name):
        os.makedirs(os.path.dirname(report_name), exist_ok=True)
    with open(report_name, 'w') as text_file:
        text_file.write('\n'.join([header] + [','.join(item) for item in results]))


def mesh_comparison(new_meshes_dir_abs, ref_meshes_dir_abs, num_processes, report_name, samples_per_model=10000,
                    dataset_file_abs=None, seed=0):
    """reference source/base/evaluation.py:307-392: the same pairing rules and the same CSV; the distances come from the
    device.  ``num_processes`` is accepted and ignored (one mesh pair takes milliseconds; HIP contexts do not fork)."""
    if not os.path.isdir(new_meshes_dir_abs):
        print('Warning: dir to check doesn\'t exist'.format(new_meshes_dir_abs))
        return
    results = []
    for a, b, code in _pairing(new_meshes_dir_abs, ref_meshes_dir_abs, dataset_file_abs):
        values = mesh_distances(a, b, samples_per_model, seed=seed) if code == 0 else (code,) * 4
        results.append((a, b) + tuple(str(x) for x in values))
    results = sorted(results, key=lambda x: x[0])
    _write_csv(report_name, 'in mesh,ref mesh,Hausdorff dist new-ref,Hausdorff dist ref-new,Hausdorff dist,'
               'Chamfer dist(-1: no input; -2: no reference)', results)
    return results


def sdf_error(rec_dir, ref_meshes_dir, report_name, device=None, sign='pseudonormal'):
    """How far the predicted SDF lies from the truth, over the WHOLE query grid (eval_predictions of the reference looks at
    the 2,000 GT queries only): for every ``rec_dir/dist_ms/<s>.xyz.npy`` + ``rec_dir/query_pts_ms/<s>.xyz.npy`` with a GT
    mesh ``ref_meshes_dir/<s>.*`` the exact signed distance of every query to the mesh (p2s_mesh_distance, clamped to
    [-1, 1] like the GT files) and, against the prediction, the MSE, the mean and max of |d_pred - d_gt| and the share of
    wrong signs.  One CSV in the style of mesh_comparison; returns its rows.  ``sign='pseudonormal'`` writes -1 for a GT
    mesh that is not closed; ``sign='winding'`` signs every mesh by the generalised winding number; ``sign='auto'`` takes
    the pseudonormal unless the mesh is open or intersects itself inside one component (gt_sdf.auto_sign)."""
    from . import gt_sdf as _gt
    if sign not in _gt.SIGNS:
        raise ValueError('sign must be one of %s (got %r)' % (_gt.SIGNS, sign))
    dev = _dev(device)
    dist_dir, pts_dir = os.path.join(rec_dir, 'dist_ms'), os.path.join(rec_dir, 'query_pts_ms')
    ref_files = sorted(f for f in os.listdir(ref_meshes_dir) if os.path.isfile(os.path.join(ref_meshes_dir, f)))
    results = []
    for name in sorted(f for f in os.listdir(dist_dir) if f.endswith('.xyz.npy')):
        f_pts = os.path.join(pts_dir, name)
        match = [f for f in ref_files if f.split('.')[0] == name.split('.')[0]]
        if not os.path.isfile(f_pts) or not match:
            continue
        f_ref = os.path.join(ref_meshes_dir, match[0])
        mesh = _gt.load_mesh(f_ref, device=dev)
        try:
            use = _gt.auto_sign(mesh)[0] if sign == 'auto' else sign
            if use == 'pseudonormal' and not mesh.closed:
                results.append((os.path.join(dist_dir, name), f_ref, '0', '-1', '-1', '-1', '-1'))
                continue
            pred = torch.from_numpy(np.load(os.path.join(dist_dir, name)).astype(np.float64).reshape(-1)).to(dev)
            gt = mesh.distance(np.load(f_pts).astype(np.float32), signed='winding' if use == 'winding' else True).clamp_(-1.0, 1.0)
        finally:
            mesh.close()
        err = (pred - gt).abs()
        wrong = ((pred > 0) != (gt > 0)).double().mean()
        results.append((os.path.join(dist_dir, name), f_ref, str(int(gt.shape[0])), repr(float((err * err).mean())),
                        repr(float(err.mean())), repr(float(err.max())), repr(float(wrong))))
    if len(results) == 0:
        raise ValueError('Results are empty!')
    if os.path.dirname(report_name):
        os.makedirs(os.path.dirname(report_name), exist_ok=True)
    csv_lines = ['dist file,ref mesh,queries,MSE,mean abs error,max abs error,wrong sign share(-1: mesh not closed)']
    csv_lines += [','.join(item) for item in results]
    with open(report_name, 'w') as text_file:
        text_file.write('\n'.join(csv_lines))
    return results


# ---- reconstruction quality: accuracy / completeness, F-score, normal consistency, volumetric IoU
QUALITY_NOTES = ('', 'new mesh not closed', 'ref mesh not closed', 'empty union', 'too many undecided voxels')


def _read_mesh(path, dev):
    """(verts, faces) device tensors of a mesh file, or None: missing, empty or malformed (the -1 convention of
    mesh_distances; out-of-range indices never reach the device)"""
    try:
        v, f = _ply.read_ply(path)
    except Exception:
        return None
    f = np.asarray(f)
    if v.shape[0] == 0 or f.shape[0] == 0 or f.ndim != 2 or f.shape[1] != 3 or f.min() < 0 or f.max() >= v.shape[0] or \
            not np.isfinite(v).all():
        return None
    return (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).to(dev))


def surface_stats(mesh_from, mesh_to, dist, face_from, face_to, taus):
    """p2s_surface_stats: dict(sum, sum_sq, max, sum_nc, nc_pairs, counts [len(taus)]) of n samples of ``mesh_from``
    (``face_from``: their own faces) with the unsigned distances ``dist`` and the nearest faces ``face_to`` on ``mesh_to``"""
    n, t = int(dist.shape[0]), len(taus)
    d = dist.to(mesh_from.device, torch.float64).contiguous()
    ff = face_from.to(mesh_from.device, torch.int32).contiguous()
    ft = face_to.to(mesh_from.device, torch.int32).contiguous()
    out, pairs = (ctypes.c_double * (4 + t))(), ctypes.c_int64(0)
    with torch.cuda.device(mesh_from.device):
        _lib.check(mesh_from.lib.p2s_surface_stats(mesh_from.handle, mesh_to.handle, _engine._ptr(d), _engine._ptr(ff), _engine._ptr(ft),
                                                   n, (ctypes.c_double * max(t, 1))(*[float(x) for x in taus]), t, out,
                                                   ctypes.byref(pairs), _engine._stream_ptr(mesh_from.device)))
    return dict(sum=out[0], sum_sq=out[1], max=out[2], sum_nc=out[3], nc_pairs=int(pairs.value),
                counts=[int(out[4 + k]) for k in range(t)])


def occupancy_counts(occ_a, occ_b):
    """p2s_occupancy_counts: (|A|, |B|, |A and B|) of two uint8 occupancy tensors of one shape"""
    if occ_a.shape != occ_b.shape or occ_a.dtype != torch.uint8 or occ_b.dtype != torch.uint8:
        raise ValueError('two uint8 tensors of one shape')
    a, b = occ_a.contiguous(), occ_b.to(occ_a.device).contiguous()
    c = (ctypes.c_int64 * 3)()
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().p2s_occupancy_counts(_engine._ptr(a), _engine._ptr(b), int(a.numel()), c, a.device.index,
                                                    _engine._stream_ptr(a.device)))
    return int(c[0]), int(c[1]), int(c[2])


def quality_keys(taus):
    """the keys of mesh_quality's dict, in the order of the CSV columns"""
    per_tau = [k + '@%g' % t for t in taus for k in ('precision', 'recall', 'fscore')]
    return ['accuracy_mean', 'accuracy_rms', 'accuracy_max', 'completeness_mean', 'completeness_rms', 'completeness_max',
            'chamfer_l1', 'hausdorff'] + per_tau + ['normal_consistency', 'iou', 'note', 'samples', 'iou_res']


def mesh_quality(file_in, file_ref, samples_per_model=100000, taus=(0.005, 0.01), iou_res=128, seed=0, device=None):
    """How good the reconstructed mesh ``file_in`` is against ``file_ref``, as later papers report it.  From each mesh
    ``samples_per_model`` area-weighted samples with their faces (one seeded Rng, ``file_in`` first), and the EXACT
    distance of each set to the other mesh's surface (p2s_mesh_distance, unsigned):
    accuracy_* = mean / RMS / max of new -> ref, completeness_* = of ref -> new, chamfer_l1 = the mean of the two means,
    hausdorff = the larger max; per threshold tau precision = the share of new samples with d <= tau, recall = of ref
    samples, fscore = 2 P R / (P + R) (0 when P + R = 0); normal_consistency = the mean of the two mean |n . n| between a
    sample's own face and the nearest face of the other mesh (stored unit normals; pairs with a degenerate face left
    out); iou = |A and B| / |A or B| of the two voxelisations at ``iou_res`` (TriMesh.voxelize), or -1 with ``note`` saying
    why: a mesh is not closed, the union is empty, or a voxelisation has more undecided voxels than its default
    max_fallback.  The defaults are definitions (0.01 = 1 % of the unit cube's side).  A missing, empty or malformed mesh:
    every number -1."""
    from . import gt_sdf as _gt
    dev = _dev(device)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    taus = tuple(float(t) for t in taus)
    keys = quality_keys(taus)
    out = dict((k, -1.0) for k in keys)
    out.update(note='', samples=int(samples_per_model), iou_res=int(iou_res))
    rng = _engine.Rng(seed, device=dev)
    loaded = [_read_mesh(path, dev) for path in (file_in, file_ref)]
    if loaded[0] is None or loaded[1] is None:
        out['note'] = 'no input'
        return out
    meshes = [_gt.TriMesh(v, f, device=dev) for v, f in loaded]
    try:
        samples = [sample_surface(v, f, samples_per_model, rng, want_faces=True) for v, f in loaded]
        stats = []
        for src, dst in ((0, 1), (1, 0)):                      # new -> ref (accuracy), ref -> new (completeness)
            d, face_to = meshes[dst].distance(samples[src][0], signed=False, want_face=True)
            stats.append(surface_stats(meshes[src], meshes[dst], d, samples[src][2], face_to, taus))
        n = float(samples_per_model)
        for name, st in zip(('accuracy', 'completeness'), stats):
            out[name + '_mean'], out[name + '_rms'], out[name + '_max'] = st['sum'] / n, float(np.sqrt(st['sum_sq'] / n)), st['max']
        out['chamfer_l1'] = (out['accuracy_mean'] + out['completeness_mean']) / 2.0
        out['hausdorff'] = max(out['accuracy_max'], out['completeness_max'])
        for k, t in enumerate(taus):
            p, r = stats[0]['counts'][k] / n, stats[1]['counts'][k] / n
            out['precision@%g' % t], out['recall@%g' % t] = p, r
            out['fscore@%g' % t] = 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0
        nc = [st['sum_nc'] / st['nc_pairs'] if st['nc_pairs'] > 0 else -1.0 for st in stats]
        out['normal_consistency'] = (nc[0] + nc[1]) / 2.0 if min(nc) >= 0.0 else -1.0
        closed = [m.closed for m in meshes]
        if not closed[0] or not closed[1]:
            out['note'] = QUALITY_NOTES[1 if not closed[0] else 2]
        else:
            try:
                na, nb, nab = occupancy_counts(meshes[0].voxelize(iou_res), meshes[1].voxelize(iou_res))
                if na + nb - nab == 0:
                    out['note'] = QUALITY_NOTES[3]
                else:
                    out['iou'] = nab / float(na + nb - nab)
            except _lib.P2SError as e:
                if e.code != _lib.P2S_ECAPACITY:
                    raise
                out['note'] = QUALITY_NOTES[4]
    finally:
        for m in meshes:
            m.close()
    return out


def quality_comparison(new_meshes_dir_abs, ref_meshes_dir_abs, report_name, dataset_file_abs=None, **kw):
    """mesh_quality for every pair that mesh_comparison would compare (the same pairing rules, -1 for a mesh of the set that
    was never reconstructed, -2 for a reconstruction outside it): one CSV row per pair under a header naming every column,
    each row with the samples and the IoU resolution used.  ``kw``: samples_per_model, taus, iou_res, seed, device.
    Returns the rows."""
    if not os.path.isdir(new_meshes_dir_abs):
        print('Warning: dir to check doesn\'t exist'.format(new_meshes_dir_abs))
        return
    keys = quality_keys(tuple(float(t) for t in kw.get('taus', (0.005, 0.01))))
    results = []
    for a, b, code in _pairing(new_meshes_dir_abs, ref_meshes_dir_abs, dataset_file_abs):
        if code == 0:
            q = mesh_quality(a, b, **kw)
        else:
            q = dict((k, code) for k in keys)
            q.update(note='no input' if code == -1 else 'no reference', samples=int(kw.get('samples_per_model', 100000)),
                     iou_res=int(kw.get('iou_res', 128)))
        results.append((a, b) + tuple(q[k] if k == 'note' else repr(q[k]) for k in keys))
    results = sorted(results, key=lambda x: x[0])
    _write_csv(report_name, ','.join(['in mesh', 'ref mesh'] + keys) + '(-1: no input or not defined; -2: no reference)', results)
    return results


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='reconstruction quality of the meshes in --new against those in --ref: one CSV')
    ap.add_argument('--new', required=True, help='directory of the reconstructed meshes')
    ap.add_argument('--ref', required=True, help='directory of the reference meshes')
    ap.add_argument('--report', required=True, help='the CSV to write')
    ap.add_argument('--samples', type=int, default=100000, help='surface samples per mesh')
    ap.add_argument('--tau', type=float, action='append', help='F-score threshold (repeatable; default 0.005 and 0.01)')
    ap.add_argument('--iou_res', type=int, default=128, help='voxels per axis of the IoU grid')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--dataset', default=None, help='file with the names of the shapes to compare')
    opt = ap.parse_args(argv)
    for row in quality_comparison(opt.new, opt.ref, opt.report, dataset_file_abs=opt.dataset, samples_per_model=opt.samples,
                                  taus=tuple(opt.tau) if opt.tau else (0.005, 0.01), iou_res=opt.iou_res, seed=opt.seed) or ():
        print(','.join(row))


if __name__ == '__main__':
    main()
