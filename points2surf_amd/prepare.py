"""Raw scans -> a data set the engine reads (what make_pc_dataset.py does in the reference, made robust and
repeatable): drop non-finite points, crop gross strays, remove statistical outliers, thin to a budget, normalise to the unit
cube -- and ``restore`` a reconstruction into the scan's own frame.  An opt-in stage between the outliers and the thinning removes
small floating clusters (``min_cluster``; p2s_prepare_clusters).  Everything runs on the device through libp2s_hip.so
(p2s_prepare_*); torch tensors are containers only; no CPU fallback.

    python -m points2surf_amd.prepare --indir RAW --outdir DATASET [--stage prepare|restore|all] [options]
"""
import argparse
import csv
import ctypes
import os
import sys

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import file_utils

P2S_EFLAT = -7
THIN = ('random', 'voxel')
DEFAULTS = dict(crop_quantile=0.01, crop_margin=1.0, k=16, std_ratio=2.0, max_points=150000, thin='random', seed=42,
                min_cluster=0, cluster_radius=0.0, cluster_factor=3.0)
EXTENSIONS = ('.ply', '.off', '.obj', '.stl', '.xyz', '.txt', '.npy')
REPORT_COLUMNS = ('file', 'points_in', 'nonfinite', 'cropped', 'outliers', 'thinned', 'points_out', 'R', 'mean', 'std', 'threshold',
                  'centre_x', 'centre_y', 'centre_z', 'scale', 'refused')
CLUSTER_REPORT_FILE = 'clusters_report.csv'
CLUSTER_REPORT_COLUMNS = ('file', 'clusters', 'removed_clusters', 'removed_points', 'radius')


class Refused(ValueError):
    """a cloud that cannot become a data set entry; ``reason`` goes into the report"""
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


def _points(points, device=None):
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(np.array(points, dtype=np.float32, order='C'))     # a copy: read-only arrays are welcome
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError('points must be [n, 3] (got %s)' % (tuple(points.shape),))
    if device is None:
        device = points.device if points.is_cuda else torch.device('cuda', torch.cuda.current_device())
    return points.to(device, torch.float32).contiguous()


def _select(name, pts, *args, tail=()):
    """one selecting stage: (points [m, 3], ids int32 [m] into ``pts``)"""
    lib = _lib.load()
    n = pts.shape[0]
    out = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    ids = torch.empty((n,), dtype=torch.int32, device=pts.device)
    if n == 0:                                       # nothing to select from (an empty tensor has no address)
        return out, ids
    m = ctypes.c_int64(0)
    with torch.cuda.device(pts.device):
        _lib.check(getattr(lib, name)(_engine._ptr(pts), n, *args, _engine._ptr(out), _engine._ptr(ids), ctypes.byref(m), *tail,
                                      pts.device.index, _engine._stream_ptr(pts.device)))
    return out[:m.value], ids[:m.value]


def drop_nonfinite(points, device=None):
    """(points, ids): the points whose three coordinates are finite"""
    return _select('p2s_prepare_finite', _points(points, device))


def crop(points, quantile=0.01, margin=1.0, want_report=False, device=None):
    """(points, ids[, report]): per axis the order statistics of rank floor(q (n - 1)) and ceil((1 - q) (n - 1)), the box
    between them widened by ``margin`` times its extent on every side; points outside are removed.  ``quantile`` 0: off.
    report: lo, hi (the order statistics), box_lo, box_hi as float64 numpy [3]"""
    pts = _points(points, device)
    b = (ctypes.c_double * 12)()
    out, ids = _select('p2s_prepare_crop', pts, float(quantile), float(margin), tail=(b,))
    if not want_report:
        return out, ids
    b = np.array(b[:], np.float64)
    return out, ids, dict(lo=b[0:3], hi=b[3:6], box_lo=b[6:9], box_hi=b[9:12])


def remove_outliers(points, k=16, std_ratio=2.0, want_report=False, device=None):
    """(points, ids[, report]): statistical outlier removal as PCL and Open3D define it, exact: d_i = the mean distance of
    point i to its ``k`` nearest other points (``k`` clamped to n - 1), kept iff d_i <= mean + std_ratio * std over the
    cloud.  ``std_ratio`` 0: off.  report: d (float64 device tensor [n], None where the stage did not run), mean, std,
    threshold, k"""
    pts = _points(points, device)
    n = pts.shape[0]
    ran = float(std_ratio) != 0.0 and n >= 2
    d = torch.empty((n,), dtype=torch.float64, device=pts.device) if want_report and ran else None
    info = (ctypes.c_double * 4)()
    lib = _lib.load()
    out = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    ids = torch.empty((n,), dtype=torch.int32, device=pts.device)
    m = ctypes.c_int64(0)
    with torch.cuda.device(pts.device):
        if n:
            _lib.check(lib.p2s_prepare_outliers(_engine._ptr(pts), n, int(k), float(std_ratio), _engine._ptr(d), _engine._ptr(out),
                                                _engine._ptr(ids), ctypes.byref(m), info, pts.device.index,
                                                _engine._stream_ptr(pts.device)))
    out, ids = out[:m.value], ids[:m.value]
    if not want_report:
        return out, ids
    return out, ids, dict(d=d, mean=info[0], std=info[1], threshold=info[2], k=int(info[3]))


def voxel_thin(points, max_points=None, resolution=None, want_report=False, device=None):
    """(points, ids[, report]): at most one point per cell of an R^3 grid over the bounding cube, the one closest to the
    cell's centre (lowest id of equal ones), in input order.  ``resolution`` gives R (1 .. 1024); without it R is searched so
    that at most ``max_points`` cells are occupied, and a cloud of no more than ``max_points`` points comes back as it is.
    report: R (0: untouched), occupied"""
    if resolution is None and (max_points is None or int(max_points) < 1):
        raise ValueError('voxel_thin needs max_points >= 1 or a resolution')
    if resolution is not None and not 1 <= int(resolution) <= 1024:
        raise ValueError('resolution %r outside 1 .. 1024' % (resolution,))
    pts = _points(points, device)
    info = (ctypes.c_int64 * 2)()
    out, ids = _select('p2s_prepare_voxel_thin', pts, int(max_points or 0), int(resolution or 0), tail=(info,))
    return (out, ids, dict(R=int(info[0]), occupied=int(info[1]))) if want_report else (out, ids)


def remove_small_clusters(points, radius, min_points, want_report=False, device=None):
    """(points, ids[, report]): points i != j are linked iff (dx dx + dy dy) + dz dz <= radius * radius in float64; a cluster is
    a class of the transitive closure, kept iff its size >= min(min_points, size of the largest cluster) -- the largest always
    survives.  report: clusters, largest (its size), largest_label (the smallest point id of it), removed_clusters, labels
    (int32 device tensor [n]: the smallest point id of every point's cluster)"""
    radius, min_points = float(radius), int(min_points)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError('radius must be a positive finite number (got %r)' % (radius,))
    if min_points < 1:
        raise ValueError('min_points must be >= 1 (got %r)' % (min_points,))
    pts = _points(points, device)
    labels = torch.empty((pts.shape[0],), dtype=torch.int32, device=pts.device) if want_report else None
    info = (ctypes.c_int64 * 4)()
    out, ids = _select('p2s_prepare_clusters', pts, radius, min_points, _engine._ptr(labels) if want_report and pts.shape[0] else None,
                       tail=(info,))
    if not want_report:
        return out, ids
    return out, ids, dict(clusters=int(info[0]), largest=int(info[1]), largest_label=int(info[2]), removed_clusters=int(info[3]),
                          labels=labels)


def gather(src, ids):
    """rows ``ids`` (int32 device tensor) of the float32 / int32 device tensor ``src`` ([n] or [n, w])"""
    lib = _lib.load()
    if src.dtype not in (torch.float32, torch.int32):
        raise ValueError('gather moves float32 or int32 rows (got %s)' % src.dtype)
    src = src.contiguous()
    ids = ids.to(src.device, torch.int32).contiguous()
    width = 1 if src.ndim == 1 else int(src.shape[1])
    out = torch.empty((ids.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.p2s_prepare_gather(_engine._ptr(src), src.shape[0], width, _engine._ptr(ids), ids.shape[0], _engine._ptr(out),
                                          src.device.index, _engine._stream_ptr(src.device)))
    return out


def random_thin(points, max_points, seed=42, device=None):
    """(points, ids): the reference's rule, repeatable: ``RandomState(seed).choice(n, max_points, replace=False)`` in the
    order drawn (one host permutation: set-up, like train.epoch_order), gathered on the device"""
    pts = _points(points, device)
    n = pts.shape[0]
    if n <= int(max_points):
        return pts.clone(), torch.arange(n, dtype=torch.int32, device=pts.device)
    ids = np.random.RandomState(int(seed)).choice(n, int(max_points), replace=False).astype(np.int32)
    ids = torch.from_numpy(ids).to(pts.device)
    return gather(pts, ids), ids


def normalize(points, device=None):
    """(points float32 [n, 3] in the unit cube, frame): c = (lo + hi) * 0.5, s = 1 / max extent, p' = (p - c) * s in float64,
    rounded once.  frame: centre float64 numpy [3], scale float.  A cloud of coincident points raises ``Refused``"""
    pts = _points(points, device)
    lib = _lib.load()
    out = torch.empty_like(pts)
    info = (ctypes.c_double * 4)()
    with torch.cuda.device(pts.device):
        rc = lib.p2s_prepare_normalize(_engine._ptr(pts), pts.shape[0], _engine._ptr(out), info, pts.device.index,
                                       _engine._stream_ptr(pts.device))
    if rc == P2S_EFLAT:
        raise Refused('extent 0')
    _lib.check(rc)
    return out, dict(centre=np.array(info[:3], np.float64), scale=float(info[3]))


def restore(vertices, frame, device=None):
    """float64 device tensor [n, 3] = v / scale + centre: vertices of the unit cube back in the scan's own coordinates"""
    v = _points(vertices, device)
    lib = _lib.load()
    out = torch.empty(tuple(v.shape), dtype=torch.float64, device=v.device)
    c = (ctypes.c_double * 3)(*[float(x) for x in np.asarray(frame['centre'], np.float64).reshape(3)])
    with torch.cuda.device(v.device):
        _lib.check(lib.p2s_prepare_restore(_engine._ptr(v), v.shape[0], c, float(frame['scale']), _engine._ptr(out), v.device.index,
                                           _engine._stream_ptr(v.device)))
    return out


def prepare(points, device=None, **options):
    """(points float32 [m, 3], kept ids int32 [m] into the input, frame, report) -- device tensors, frame as ``normalize``
    gives it with ``kept`` added.  Options and defaults: ``DEFAULTS``.  The stages in order: non-finite points, crop
    (crop_quantile 0: off), outliers (std_ratio 0: off), small clusters (min_cluster 0: off; the radius is cluster_radius, or
    with 0 cluster_factor times the outlier stage's mean -- before the thinning, which changes the density that this scales
    by), thinning (max_points 0: off; only when more points are left), unit cube.  report: points_in, nonfinite, cropped,
    outliers, thinned, points_out, R, mean, std, threshold; with the cluster stage on also clusters, small_clusters (the
    clusters removed), cluster_points (the points removed with them) and cluster_radius."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError('unknown options %s' % sorted(unknown))
    o = dict(DEFAULTS, **options)
    if o['thin'] not in THIN:
        raise ValueError('thin must be one of %s (got %r)' % (THIN, o['thin']))
    if int(o['min_cluster']) < 0 or not float(o['cluster_radius']) >= 0.0 or not float(o['cluster_factor']) > 0.0:
        raise ValueError('min_cluster >= 0, cluster_radius >= 0 and cluster_factor > 0 are needed (got %r, %r, %r)'
                         % (o['min_cluster'], o['cluster_radius'], o['cluster_factor']))
    if int(o['min_cluster']) > 0 and float(o['cluster_radius']) == 0.0 and float(o['std_ratio']) == 0.0:
        raise ValueError('with the outlier stage off (std_ratio 0) the cluster stage has no density to scale by: '
                         'give --cluster_radius')
    pts = _points(points, device)
    rep = dict(points_in=int(pts.shape[0]))
    pts, kept = drop_nonfinite(pts)
    rep['nonfinite'] = rep['points_in'] - pts.shape[0]

    def stage(name, result):
        nonlocal pts, kept
        rep[name] = pts.shape[0] - result[0].shape[0]
        kept = gather(kept, result[1]) if result[1].shape[0] else kept[:0]
        pts = result[0]
        return result[2] if len(result) > 2 else None

    stage('cropped', crop(pts, o['crop_quantile'], o['crop_margin']))
    info = stage('outliers', remove_outliers(pts, o['k'], o['std_ratio'], want_report=True))
    rep.update(mean=info['mean'], std=info['std'], threshold=info['threshold'])
    if int(o['min_cluster']) > 0 and pts.shape[0] > 0:
        radius = float(o['cluster_radius']) or float(o['cluster_factor']) * float(info['mean'])
        if not radius > 0.0:
            raise Refused('cluster radius 0 (the mean neighbour distance is 0)')
        cl = stage('cluster_points', remove_small_clusters(pts, radius, int(o['min_cluster']), want_report=True))
        rep.update(clusters=cl['clusters'], small_clusters=cl['removed_clusters'], cluster_radius=radius)
    rep['R'] = 0
    if o['max_points'] and pts.shape[0] > int(o['max_points']):
        if o['thin'] == 'random':
            stage('thinned', random_thin(pts, o['max_points'], o['seed']))
        else:
            rep['R'] = stage('thinned', voxel_thin(pts, o['max_points'], want_report=True))['R']
    else:
        rep['thinned'] = 0
    if pts.shape[0] < 1:
        raise Refused('no points left')
    pts, frame = normalize(pts)
    rep['points_out'] = int(pts.shape[0])
    frame['kept'] = kept
    return pts, kept, frame, rep


# ---- files ----------------------------------------------------------------------------------------------------------------

def read_cloud(path):
    """float32 [n, 3] of a .ply / .off / .obj / .stl (vertices only), .xyz / .txt (the first three columns) or .npy file"""
    ext = os.path.splitext(path)[1].lower()
    if os.path.getsize(path) == 0:
        raise ValueError('empty file')
    if ext == '.npy':
        p = np.load(path)
    elif ext == '.ply':
        from . import ply
        p = ply.read_ply(path)[0]
    elif ext in ('.off', '.obj', '.stl'):
        from . import mesh_formats
        p = mesh_formats.read_mesh(path)[0]
    elif ext in ('.xyz', '.txt'):
        p = np.loadtxt(path, dtype=np.float64, ndmin=2)
    else:
        raise ValueError('unknown extension %r' % ext)
    p = np.asarray(p)
    if p.ndim != 2 or p.shape[1] < 3 or p.shape[0] < 1:
        raise ValueError('no [n, 3] points (shape %s)' % (tuple(p.shape),))
    return np.ascontiguousarray(p[:, :3], dtype=np.float32)


def _stem(name):
    return os.path.splitext(name)[0]


def _row(name, rep=None, frame=None, refused=''):
    row = dict.fromkeys(REPORT_COLUMNS, '')
    row.update(file=name, refused=refused)
    for key in REPORT_COLUMNS:
        if rep and key in rep:
            row[key] = repr(rep[key]) if isinstance(rep[key], float) else rep[key]
    if frame:
        row.update(centre_x=repr(float(frame['centre'][0])), centre_y=repr(float(frame['centre'][1])),
                   centre_z=repr(float(frame['centre'][2])), scale=repr(float(frame['scale'])))
    return row


def prepare_dir(indir, outdir, device=None, **options):
    """every cloud of ``indir`` -> <outdir>/04_pts/<stem>.xyz.npy, 04_pts_frame/<stem>.npz, testset.txt, prepare_report.csv;
    a refused file gets its reason in the report and does not stop the run.  Returns the report rows."""
    o = dict(DEFAULTS, **options)
    pts_dir, frame_dir = os.path.join(outdir, '04_pts'), os.path.join(outdir, '04_pts_frame')
    os.makedirs(pts_dir, exist_ok=True)
    os.makedirs(frame_dir, exist_ok=True)
    report_path = os.path.join(outdir, 'prepare_report.csv')
    old = {}
    if os.path.isfile(report_path):
        with open(report_path, newline='') as f:
            old = {r['file']: r for r in csv.DictReader(f)}
    rows, written, cluster_rows, old_clusters = [], [], [], {}
    if os.path.isfile(os.path.join(outdir, CLUSTER_REPORT_FILE)):
        with open(os.path.join(outdir, CLUSTER_REPORT_FILE), newline='') as f:
            old_clusters = {r['file']: r for r in csv.DictReader(f)}
    for name in sorted(f for f in os.listdir(indir) if os.path.splitext(f)[1].lower() in EXTENSIONS):
        src, stem = os.path.join(indir, name), _stem(name)
        out_pts, out_frame = os.path.join(pts_dir, stem + '.xyz.npy'), os.path.join(frame_dir, stem + '.npz')
        if name in old and not old[name].get('refused') and not file_utils.call_necessary([src], [out_pts, out_frame]):
            print('up to date: %s' % name)
            rows.append(old[name])
            written.append(stem)
            if name in old_clusters:
                cluster_rows.append(old_clusters[name])
            continue
        try:
            raw = read_cloud(src)
        except Exception as e:      # whatever a reader makes of a broken file: the run goes on
            rows.append(_row(name, refused='unreadable: %s' % (str(e).splitlines() or [type(e).__name__])[0]))
            continue
        try:
            pts, kept, frame, rep = prepare(raw, device=device, **o)
            if pts.shape[0] < int(o['k']) + 1:
                raise Refused('fewer than k + 1 = %d points left (%d)' % (int(o['k']) + 1, pts.shape[0]))
        except Refused as e:
            rows.append(_row(name, dict(points_in=int(raw.shape[0])), refused=e.reason))
            continue
        np.save(out_pts, pts.cpu().numpy())
        np.savez(out_frame, centre=frame['centre'], scale=np.float64(frame['scale']), kept=kept.cpu().numpy().astype(np.int32))
        rows.append(_row(name, rep, frame))
        written.append(stem)
        if 'clusters' in rep:
            cluster_rows.append(dict(file=name, clusters=rep['clusters'], removed_clusters=rep['small_clusters'],
                                     removed_points=rep['cluster_points'], radius=repr(rep['cluster_radius'])))
    with open(os.path.join(outdir, 'testset.txt'), 'w') as f:
        f.write(''.join(s + '\n' for s in sorted(written)))
    with open(report_path, 'w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=REPORT_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    if int(o['min_cluster']) > 0:                    # the cluster stage reports in a file of its own: prepare_report.csv stays as it was
        with open(os.path.join(outdir, CLUSTER_REPORT_FILE), 'w', newline='') as f:
            w = csv.DictWriter(f, fieldnames=CLUSTER_REPORT_COLUMNS)
            w.writeheader()
            w.writerows(cluster_rows)
    return rows


def restore_dir(outdir, meshes, restored, device=None):
    """every <meshes>/<stem>.ply with a frame in <outdir>/04_pts_frame -> <restored>/<stem>.ply in the scan's own
    coordinates; returns the stems written"""
    from . import ply
    os.makedirs(restored, exist_ok=True)
    done = []
    for name in sorted(f for f in os.listdir(meshes) if f.lower().endswith('.ply')):
        stem = _stem(name)
        frame_path, src, dst = os.path.join(outdir, '04_pts_frame', stem + '.npz'), os.path.join(meshes, name), os.path.join(restored, name)
        if not os.path.isfile(frame_path):
            print('WARNING: no frame for %s' % name)
            continue
        if not file_utils.call_necessary([src, frame_path], [dst]):
            print('up to date: %s' % name)
            done.append(stem)
            continue
        v, faces = ply.read_ply(src)
        with np.load(frame_path) as z:
            frame = dict(centre=z['centre'], scale=float(z['scale']))
        out = restore(np.asarray(v, np.float32), frame, device=device).cpu().numpy() if len(v) else np.zeros((0, 3))
        ply.write_ply(dst, out, faces if len(faces) else None)
        done.append(stem)
    return done


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m points2surf_amd.prepare', description=__doc__.split('\n\n')[0])
    ap.add_argument('--indir', help='directory of raw clouds (%s)' % ' '.join(EXTENSIONS))
    ap.add_argument('--outdir', required=True, help='the data set: 04_pts, 04_pts_frame, testset.txt, prepare_report.csv')
    ap.add_argument('--stage', choices=('prepare', 'restore', 'all'), default='prepare')
    ap.add_argument('--crop_quantile', type=float, default=DEFAULTS['crop_quantile'], help='0: no crop')
    ap.add_argument('--crop_margin', type=float, default=DEFAULTS['crop_margin'])
    ap.add_argument('--k', type=int, default=DEFAULTS['k'])
    ap.add_argument('--std_ratio', type=float, default=DEFAULTS['std_ratio'], help='0: no outlier removal')
    ap.add_argument('--max_points', type=int, default=DEFAULTS['max_points'], help='0: no thinning')
    ap.add_argument('--thin', choices=THIN, default=DEFAULTS['thin'])
    ap.add_argument('--seed', type=int, default=DEFAULTS['seed'])
    ap.add_argument('--min_cluster', type=int, default=DEFAULTS['min_cluster'],
                    help='remove the clusters of fewer points (the largest always stays); 0: off')
    ap.add_argument('--cluster_radius', type=float, default=DEFAULTS['cluster_radius'],
                    help='two points within this distance are linked; 0: --cluster_factor times the mean neighbour distance')
    ap.add_argument('--cluster_factor', type=float, default=DEFAULTS['cluster_factor'], help='a choice, not a measurement')
    ap.add_argument('--meshes', help='restore: directory of <stem>.ply reconstructions in the unit cube')
    ap.add_argument('--restored', help='restore: where the meshes in the scans\' own coordinates go')
    ap.add_argument('--gpu_idx', type=int, default=0)
    a = ap.parse_args(argv)
    device = _engine.select_device(a.gpu_idx)
    if a.stage in ('prepare', 'all'):
        if not a.indir:
            ap.error('--stage %s needs --indir' % a.stage)
        rows = prepare_dir(a.indir, a.outdir, device=device, **{key: getattr(a, key) for key in DEFAULTS})
        print('%d files, %d refused' % (len(rows), sum(1 for r in rows if r['refused'])))
    if a.stage in ('restore', 'all'):
        if not a.meshes or not a.restored:
            ap.error('--stage %s needs --meshes and --restored' % a.stage)
        print('%d meshes restored' % len(restore_dir(a.outdir, a.meshes, a.restored, device=device)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
