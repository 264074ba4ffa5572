"""Connected components of triangle meshes on the device, and the removal of floating debris: the small
closed blobs and inner cavities that a few wrong signs leave in an iso-surface.  It runs in libp2s_hip.so
(p2s_mesh_components, p2s_mesh_submesh); the definitions are in include/p2s_hip.h.  This is the project's own definition --
not trimesh's ``split`` and not MeshLab's "remove isolated pieces".  Faces are connected through shared vertex INDICES:
unwelded input (equal coordinates under different indices) is out of contract, weld it with ``clean`` first.  Torch tensors
are containers only; no CPU fallback.

``python -m points2surf_amd.components --indir DIR --outdir DIR2 [--min_faces N] [--min_area_share S] [--max_components K]
[--dataset FILE] [--gpu_idx I]`` reads every mesh of ``DIR`` that mesh_formats can read (with ``--dataset``: the shapes that the
list names), writes ``DIR2/<stem>.ply`` and ``DIR2/components_report.csv`` with one row per mesh.  A mesh whose output is newer
than its input keeps its file and its row.  A mesh that fails is named in the report with the reason; the run goes on.
"""
import argparse
import csv
import ctypes
import math
import os
import sys

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import file_utils
from . import mesh_formats as _formats
from . import ply as _ply
from . import prepare as _prepare
from .simplify import _device, _names

P2S_EINVAL = -1
FIRST_CAP = 65536
STAT_KEYS = ('first_face', 'faces', 'vertices', 'boundary_edges', 'nonmanifold_edges', 'area', 'volume', 'box_lo', 'box_hi', 'closed')
SELECT_DEFAULTS = dict(min_faces=0, min_area_share=0.0, max_components=0)
REPORT_FILE = 'components_report.csv'
REPORT_COLUMNS = ('mesh', 'components', 'components_kept', 'faces_in', 'faces_out', 'verts_in', 'verts_out', 'area_in', 'area_out',
                  'closed_components', 'cavities', 'largest_removed_area_share', 'verdict')


def report_dict(a):
    """the int64[8] report of p2s_mesh_components as a dict"""
    a = [int(x) for x in a]
    m = (1 << 32) - 1
    return dict(verts_in=a[0] & m, faces_in=a[0] >> 32, components=a[1], largest_faces=a[2], largest_area_rank=a[3],
                unreferenced_vertices=a[4], hook_rounds=a[5])


def _mesh(verts, faces, dev):
    if isinstance(verts, np.ndarray):
        verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
    v = verts.to(dev, torch.float32).contiguous()
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError('verts must be [V, 3] (got %s)' % (tuple(v.shape),))
    if isinstance(faces, np.ndarray):
        faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int32))
    f = faces.to(dev, torch.int32).contiguous()
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('faces must be [F, 3] (got %s)' % (tuple(f.shape),))
    return v, f


def _ptr(t):
    return _engine._ptr(t) if t is not None and t.numel() else None


def stats_dict(counts, measures):
    """``counts`` int64 [C, 5] and ``measures`` float64 [C, 8] of p2s_mesh_components as a dict of numpy arrays (STAT_KEYS)"""
    counts = np.asarray(counts, np.int64).reshape(-1, 5)
    measures = np.asarray(measures, np.float64).reshape(-1, 8)
    return dict(first_face=counts[:, 0].copy(), faces=counts[:, 1].copy(), vertices=counts[:, 2].copy(),
                boundary_edges=counts[:, 3].copy(), nonmanifold_edges=counts[:, 4].copy(), area=measures[:, 0].copy(),
                volume=measures[:, 1].copy(), box_lo=measures[:, 2:5].copy(), box_hi=measures[:, 5:8].copy(),
                closed=(counts[:, 3] == 0) & (counts[:, 4] == 0))


def components(verts, faces, device=None):
    """``verts`` [V, 3] float32, ``faces`` [F, 3] int32 (numpy arrays or tensors) -> (comp, stats, report): ``comp`` the int32
    device tensor [F] of every face's component (its rank in the order of the components' smallest face ids), ``stats`` a
    dict of numpy arrays over the C components (STAT_KEYS; ``closed``: no boundary edge and no edge of more than two faces),
    ``report`` the dict of ``report_dict``"""
    dev = _device(device)
    lib = _lib.load()
    v, f = _mesh(verts, faces, dev)
    V, F = int(v.shape[0]), int(f.shape[0])
    comp = torch.empty((F,), dtype=torch.int32, device=dev)
    rep = (ctypes.c_int64 * 8)()
    cap = min(F, FIRST_CAP)
    with torch.cuda.device(dev):
        while True:
            counts = torch.empty((cap, 5), dtype=torch.int64, device=dev)
            meas = torch.empty((cap, 8), dtype=torch.float64, device=dev)
            rc = lib.p2s_mesh_components(_ptr(v), V, _ptr(f), F, _ptr(comp), cap, _ptr(counts), _ptr(meas), rep, dev.index,
                                         _engine._stream_ptr(dev))
            if rc == P2S_EINVAL and int(rep[1]) > cap:              # the capacity refusal: the report holds the exact count
                cap = int(rep[1])
                continue
            _lib.check(rc)
            break
    r = report_dict(rep)
    C = r['components']
    return comp, stats_dict(counts[:C].cpu().numpy(), meas[:C].cpu().numpy()), r


def select(stats, min_faces=0, min_area_share=0.0, max_components=0):
    """bool [C]: the components to keep.  Kept iff ``faces >= min_faces`` and ``area >= min_area_share * max(area)`` (float64);
    with ``max_components > 0`` of those the ``max_components`` of largest area, of equal areas the smaller ``first_face``
    first.  The component of largest area (of equal ones the first) is always kept.  Host arithmetic over C numbers."""
    if int(min_faces) < 0 or int(max_components) < 0:
        raise ValueError('min_faces and max_components must be >= 0 (got %r, %r)' % (min_faces, max_components))
    share = float(min_area_share)
    if not 0.0 <= share <= 1.0:
        raise ValueError('min_area_share must lie in [0, 1] (got %r)' % (min_area_share,))
    area = np.asarray(stats['area'], np.float64)
    C = area.shape[0]
    if C == 0:
        return np.zeros((0,), bool)
    keep = (np.asarray(stats['faces'], np.int64) >= int(min_faces)) & (area >= np.float64(share) * area.max())
    order = np.lexsort((np.asarray(stats['first_face'], np.int64), -area))      # largest area first, then the smaller first face
    keep[order[0]] = True
    if int(max_components) > 0:
        chosen = [c for c in order if keep[c]][:int(max_components)]
        keep = np.zeros((C,), bool)
        keep[chosen] = True
    return keep


def submesh(verts, faces, keep_faces, device=None, want_map=False):
    """the faces whose ``keep_faces`` entry (bool or integer, [F], numpy or tensor) is nonzero, in input order, with the
    vertices they reference -> (verts, faces, report): device tensors and dict(verts_in, faces_in, verts_out, faces_out);
    with ``want_map`` also 'vert_map' [V] int32 (-1: dropped) and 'face_src' [F'] int32"""
    dev = _device(device)
    lib = _lib.load()
    v, f = _mesh(verts, faces, dev)
    V, F = int(v.shape[0]), int(f.shape[0])
    if isinstance(keep_faces, np.ndarray):
        keep_faces = torch.from_numpy(np.ascontiguousarray(keep_faces != 0).astype(np.int32))
    k = keep_faces.to(dev, torch.int32).contiguous()
    if tuple(k.shape) != (F,):
        raise ValueError('keep_faces must be [%d] (got %s)' % (F, tuple(k.shape)))
    vo = torch.empty((V, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((F, 3), dtype=torch.int32, device=dev)
    so = torch.empty((F,), dtype=torch.int32, device=dev) if want_map else None
    mo = torch.empty((V,), dtype=torch.int32, device=dev) if want_map else None
    rep = (ctypes.c_int64 * 3)()
    with torch.cuda.device(dev):
        _lib.check(lib.p2s_mesh_submesh(_ptr(v), V, _ptr(f), F, _ptr(k), _ptr(vo), V, _ptr(fo), _ptr(so), F, _ptr(mo), rep, dev.index,
                                        _engine._stream_ptr(dev)))
    r = dict(verts_in=V, faces_in=F, verts_out=int(rep[1]), faces_out=int(rep[2]))
    if want_map:
        r['vert_map'] = mo
        r['face_src'] = so[:r['faces_out']]
    return vo[:r['verts_out']], fo[:r['faces_out']], r


def face_mask(comp, keep):
    """the int32 device mask [F] of the faces whose component ``keep`` (bool [C]) keeps: a gather on the device"""
    table = torch.from_numpy(np.ascontiguousarray(keep).astype(np.int32)).to(comp.device)
    if comp.shape[0] == 0:
        return torch.empty((0,), dtype=torch.int32, device=comp.device)
    return _prepare.gather(table, comp)


def filter_mesh(verts, faces, device=None, **options):
    """the mesh without the components that ``select(stats, **options)`` drops -> (verts, faces, report); the report holds
    the counts of ``submesh`` and 'components', 'components_kept', 'keep' (bool [C]), 'stats', 'area_in', 'area_out',
    'closed_components', 'cavities' (closed components of negative volume) and 'largest_removed_area_share'"""
    unknown = set(options) - set(SELECT_DEFAULTS)
    if unknown:
        raise TypeError('unknown options %s' % sorted(unknown))
    dev = _device(device)
    v, f = _mesh(verts, faces, dev)
    comp, stats, _ = components(v, f, device=dev)
    keep = select(stats, **options)
    vo, fo, r = submesh(v, f, face_mask(comp, keep), device=dev)
    area = stats['area']
    area_in = math.fsum(area.tolist())
    removed = area[~keep]
    r.update(components=int(keep.shape[0]), components_kept=int(keep.sum()), keep=keep, stats=stats, area_in=area_in,
             area_out=math.fsum(area[keep].tolist()), closed_components=int(stats['closed'].sum()),
             cavities=int((stats['closed'] & (stats['volume'] < 0.0)).sum()),
             largest_removed_area_share=float(removed.max() / area_in) if removed.size and area_in > 0.0 else 0.0)
    return vo, fo, r


def filter_file(file_in, file_out, device=None, **options):
    """``file_in`` (any type of mesh_formats) filtered into the PLY ``file_out``; the report of ``filter_mesh``"""
    v, f = _formats.read_mesh(file_in)
    dev = _device(device)
    vo, fo, rep = filter_mesh(np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f).astype(np.int32).reshape(-1, 3),
                              device=dev, **options)
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    _ply.write_ply(file_out, vo.cpu().numpy(), fo.cpu().numpy())
    return rep


def _row(name, rep):
    return dict(mesh=name, components=rep['components'], components_kept=rep['components_kept'], faces_in=rep['faces_in'],
                faces_out=rep['faces_out'], verts_in=rep['verts_in'], verts_out=rep['verts_out'], area_in=repr(rep['area_in']),
                area_out=repr(rep['area_out']), closed_components=rep['closed_components'], cavities=rep['cavities'],
                largest_removed_area_share=repr(rep['largest_removed_area_share']), verdict='written')


def filter_dir(indir, outdir, dataset=None, device=None, **options):
    """every mesh of ``indir`` as ``outdir/<stem>.ply`` and ``outdir/components_report.csv``; a mesh whose output is newer than
    its input keeps its file and its row of the earlier report.  Returns the files written by this run."""
    os.makedirs(outdir, exist_ok=True)
    report_path = os.path.join(outdir, REPORT_FILE)
    old = {}
    if os.path.isfile(report_path):
        with open(report_path, newline='') as fh:
            old = {r['mesh']: r for r in csv.DictReader(fh)}
    written, rows = [], []
    for name in _names(indir, dataset):
        f_in, f_out = os.path.join(indir, name), os.path.join(outdir, os.path.splitext(name)[0] + '.ply')
        if old.get(name, {}).get('verdict') == 'written' and not file_utils.call_necessary([f_in], [f_out]):
            print('up to date: %s' % name)
            rows.append(old[name])
            continue
        try:
            rows.append(_row(name, filter_file(f_in, f_out, device=device, **options)))
            written.append(f_out)
        except Exception as e:                          # named in the report; the run goes on
            if os.path.isfile(f_out):
                os.remove(f_out)                        # a mesh that fails now is not left over from an earlier run
            row = dict.fromkeys(REPORT_COLUMNS, '')
            row.update(mesh=name, verdict='failed: %s' % ' '.join(str(e).split()))
            rows.append(row)
    with open(report_path, 'w', newline='') as fh:
        w = csv.DictWriter(fh, fieldnames=REPORT_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m points2surf_amd.components',
                                 description='remove the small connected components of every mesh of INDIR into OUTDIR')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--min_faces', type=int, default=0, help='drop components of fewer faces')
    ap.add_argument('--min_area_share', type=float, default=0.01,
                    help='drop components whose area is below this share of the largest component\'s (a choice, not a measurement)')
    ap.add_argument('--max_components', type=int, default=0, help='keep at most this many, by area; 0: no limit')
    ap.add_argument('--dataset', default=None, help='a list of shape names: only these meshes')
    ap.add_argument('--gpu_idx', type=int, default=0)
    opt = ap.parse_args(argv)
    select(stats_dict(np.zeros((0, 5)), np.zeros((0, 8))), opt.min_faces, opt.min_area_share, opt.max_components)      # the ranges
    device = _engine.select_device(opt.gpu_idx)
    for f in filter_dir(opt.indir, opt.outdir, dataset=opt.dataset, device=device, min_faces=opt.min_faces,
                        min_area_share=opt.min_area_share, max_components=opt.max_components):
        print(f)
    print(os.path.join(opt.outdir, REPORT_FILE))
    return 0


if __name__ == '__main__':
    sys.exit(main())
